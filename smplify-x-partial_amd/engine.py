"""Batched fitting engine: Python face of libsfx.so (the MI355X-native entry point).

`DeviceModel` uploads an SMPL-X model once per GPU; `FrameBatch` holds B independent
frames (the reference handles exactly one, fit_single_frame.py:119) and runs the
reference's per-frame schedule for all of them on device.  The drop-in modules
(`smplx`, `fitting`, `fit_single_frame`, ...) are thin adapters over these two classes.
"""
import collections
import ctypes as C
import functools

import numpy as np

from . import _args as A
from . import _capi as capi
from .synthetic import SMPLX_EXTRA_VERTEX_IDS

NUM_BODY_JOINTS = {"coco25": 25, "halpe": 26, "coco_wholebody": 23}
PARAM_NAMES = ("cam_translation", "global_orient", "betas", "left_hand_pose", "right_hand_pose",
               "expression", "jaw_pose", "leye_pose", "reye_pose", "pose_embedding")


def _jaw_weights(cfg, shape_weights):
    jw = cfg.get("jaw_pose_prior_weights")
    if jw is None:
        return [[x] * 3 for x in shape_weights]
    return [[float(v) for v in e.split(",")] if isinstance(e, str) else [float(v) for v in e] for e in jw]


def stage_weights_from_cfg(cfg, struct=None):
    """Per-stage weights exactly as fit_single_frame.py:133-207,330-353 assembles them
    (defaults, zip-truncation to the shortest list).  struct: capi.StageWeights (default) or capi.StageWeights64 (the
    float64 mode: the Python floats kept unrounded)."""
    use_hands, use_face = cfg.get("use_hands", True), cfg.get("use_face", True)
    bpw = cfg.get("body_pose_prior_weights") or [4.04 * 1e2, 4.04 * 1e2, 57.4, 4.78]
    n = len(bpw)
    lists = {"data": cfg.get("data_weights") or [1] * n, "bpw": bpw,
             "shape": cfg.get("shape_weights") or [1e2, 5 * 1e1, 1e1, .5 * 1e1]}
    if use_face:
        lists["face"] = cfg.get("face_joints_weights") or [0.0, 0.0, 0.0, 1.0]
        lists["expr"] = cfg.get("expr_weights") or [1e2, 5 * 1e1, 1e1, .5 * 1e1]
        lists["jaw"] = _jaw_weights(cfg, lists["shape"])
    if use_hands:
        lists["hand"] = cfg.get("hand_joints_weights") or [0.0, 0.0, 0.0, 1.0]
        lists["hprior"] = cfg.get("hand_pose_prior_weights") or [1e2, 5 * 1e1, 1e1, .5 * 1e1]
    if cfg.get("interpenetration", False):
        lists["coll"] = cfg.get("coll_loss_weights") or [0.0] * n
    lists["go"] = cfg.get("global_orient_weights") or [20, 10, 7.5, 5, 5]
    for k in ("shape", "face", "expr", "jaw", "hand", "hprior", "coll"):
        if k in lists and len(lists[k]) != n:
            raise AssertionError("Number of Body pose prior weights does not match the number of %s weights" % k)
    ns = min(len(v) for v in lists.values())
    out = []
    for i in range(ns):
        w = (struct or capi.StageWeights)()
        w.body_pose_weight = lists["bpw"][i]
        w.shape_weight = lists["shape"][i]
        w.hand_prior_weight = lists["hprior"][i] if use_hands else 0.0
        w.expr_prior_weight = lists["expr"][i] if use_face else 0.0
        jaw = lists["jaw"][i] if use_face else [0.0, 0.0, 0.0]
        for q in range(3):
            w.jaw_prior_weight[q] = jaw[q]
        w.hand_joint_weight = lists["hand"][i] if use_hands else 0.0
        w.face_joint_weight = lists["face"][i] if use_face else 0.0
        w.coll_loss_weight = lists["coll"][i] if "coll" in lists else 0.0
        w.bending_prior_weight = -1.0
        out.append(w)
    return out, n


class DeviceModel(capi.Handle):
    """SMPL-X constants resident in HBM (sfx_model).  `model` is a dict with the .npz key
    set of SURVEY.md appendix A.1 (a real SMPLX_*.npz loaded with numpy, or
    synthetic.make_synthetic_model())."""
    _destroy = "sfx_model_destroy"

    def __init__(self, model, joint_map=None, num_betas=10, num_expression_coeffs=10,
                 num_pca_comps=12, flat_hand_mean=False, use_face_contour=True,
                 extra_vertex_ids=None, vposer=None, use_pca=True):
        """use_pca=False (cmd_parser.py:127, smplx.SMPLX): the hand pose parameters are the 45 axis-angle values
        themselves -- the same kernels with identity 'components'."""
        lib = capi.load()
        self.use_pca = bool(use_pca)
        if not self.use_pca:
            num_pca_comps = 45
        sd = np.asarray(model["shapedirs"])
        es = 300 if sd.shape[-1] >= 400 else 10
        sdirs = np.concatenate([sd[:, :, :num_betas], sd[:, :, es:es + num_expression_coeffs]], -1)
        V = int(np.asarray(model["v_template"]).shape[0])
        faces = capi.i32(np.asarray(model["f"]).astype(np.int64))
        parents = np.asarray(model["kintree_table"])[0].astype(np.int64).copy()
        parents[0] = -1
        lm = np.zeros(45) if flat_hand_mean else np.asarray(model["hands_meanl"])
        rm = np.zeros(45) if flat_hand_mean else np.asarray(model["hands_meanr"])
        pose_mean = np.concatenate([np.zeros(75), lm, rm])
        if extra_vertex_ids is None:
            extra_vertex_ids = model.get("extra_vertex_ids", SMPLX_EXTRA_VERTEX_IDS)
        n_lmk = int(np.asarray(model["lmk_faces_idx"]).shape[0])
        dyn_f = np.asarray(model["dynamic_lmk_faces_idx"])
        n_dyn = int(dyn_f.shape[1]) if use_face_contour else 0
        n_all = 55 + len(extra_vertex_ids) + n_lmk + n_dyn
        if joint_map is None:
            joint_map = np.arange(n_all)
        self.joint_map = np.asarray(joint_map).astype(np.int64)
        self.V, self.F, self.K = V, int(faces.shape[0]), int(len(self.joint_map))
        # distinct vertices the keypoints read (extra vertices, landmark corners, every corner a dynamic landmark can land on):
        # the columns of debug_read("uvp") -- csrc/model_tables.h n_uniq
        fa, e0, l0 = np.asarray(model["f"]).astype(np.int64), 55, 55 + len(extra_vertex_ids)
        uniq = set()
        for s_ in self.joint_map:
            if e0 <= s_ < l0:
                uniq.add(int(np.asarray(extra_vertex_ids)[s_ - e0]))
            elif l0 <= s_ < l0 + n_lmk:
                uniq.update(int(v) for v in fa[int(np.asarray(model["lmk_faces_idx"])[s_ - l0])])
            elif l0 + n_lmk <= s_ < n_all:      # (an entry out of range is refused by sfx_model_create below)
                uniq.update(int(v) for v in fa[dyn_f[:, s_ - l0 - n_lmk].astype(np.int64)].ravel())
        self.n_uniq = len(uniq)
        self.num_betas, self.num_expr, self.num_pca = num_betas, num_expression_coeffs, num_pca_comps
        self.faces = np.asarray(model["f"]).astype(np.int64)
        keep = dict(
            v_template=capi.f32(model["v_template"]), shapedirs=capi.f32(sdirs),
            posedirs=capi.f32(model["posedirs"]), J_regressor=capi.f32(model["J_regressor"]),
            lbs_weights=capi.f32(model["weights"]), parents=capi.i32(parents),
            hands_comp_l=capi.f32(np.asarray(model["hands_componentsl"])[:num_pca_comps] if self.use_pca else np.eye(45)),
            hands_comp_r=capi.f32(np.asarray(model["hands_componentsr"])[:num_pca_comps] if self.use_pca else np.eye(45)),
            pose_mean=capi.f32(pose_mean), faces=faces,
            extra=capi.i32(extra_vertex_ids), lmk_f=capi.i32(model["lmk_faces_idx"]),
            lmk_b=capi.f32(model["lmk_bary_coords"]), dyn_f=capi.i32(dyn_f),
            dyn_b=capi.f32(model["dynamic_lmk_bary_coords"]), jm=capi.i32(self.joint_map))
        d = capi.ModelDesc()
        d.V, d.F, d.J = V, self.F, 55
        d.num_betas, d.num_expr, d.num_pca = num_betas, num_expression_coeffs, num_pca_comps
        d.v_template = capi.fptr(keep["v_template"]); d.shapedirs = capi.fptr(keep["shapedirs"])
        d.posedirs = capi.fptr(keep["posedirs"]); d.J_regressor = capi.fptr(keep["J_regressor"])
        d.lbs_weights = capi.fptr(keep["lbs_weights"]); d.parents = capi.iptr(keep["parents"])
        d.hands_comp_l = capi.fptr(keep["hands_comp_l"]); d.hands_comp_r = capi.fptr(keep["hands_comp_r"])
        d.pose_mean = capi.fptr(keep["pose_mean"]); d.faces = capi.iptr(keep["faces"])
        d.n_extra = len(extra_vertex_ids); d.extra_vertex_ids = capi.iptr(keep["extra"])
        d.n_lmk = n_lmk; d.lmk_faces_idx = capi.iptr(keep["lmk_f"]); d.lmk_bary = capi.fptr(keep["lmk_b"])
        d.n_dyn_rows = int(dyn_f.shape[0]) if n_dyn else 0; d.n_dyn = n_dyn
        d.dyn_lmk_faces_idx = capi.iptr(keep["dyn_f"]); d.dyn_lmk_bary = capi.fptr(keep["dyn_b"])
        d.K = self.K; d.joint_map = capi.iptr(keep["jm"])
        h = C.c_void_p()
        capi.check(lib.sfx_model_create(C.byref(d), C.byref(h)))
        self._h = h
        self._lib = lib
        self.vposer_latent = 0
        self.vposer_weights = None
        if vposer is not None:
            self.set_vposer(vposer)

    def set_parts(self, segm, parents, ign_part_pairs=None):
        """Per-face part labels (smplx_parts_segm.pkl: 'segm', 'parents') and the cfg's
        ign_part_pairs (["9,16", ...]) for batches created with interpenetration=True
        (fit_single_frame.py:316-328)."""
        sg, pr = capi.i32(np.asarray(segm).astype(np.int64)), capi.i32(np.asarray(parents).astype(np.int64))
        assert sg.shape == (self.F,) and pr.shape == (self.F,), "one label per face"
        ign = A.ign_pairs(ign_part_pairs)
        capi.check(self._lib.sfx_model_set_parts(self._h, capi.iptr(sg), capi.iptr(pr),
                                                 capi.iptr(ign) if len(ign) else None, len(ign)))
        self.has_parts = True

    def clear_parts(self):
        """No part filter (a loss created without a FilterFaces module: the reference filters nothing then)."""
        capi.check(self._lib.sfx_model_set_parts(self._h, None, None, None, 0))
        self.has_parts = False

    def set_vposer(self, w):
        a = {k: capi.f32(v) for k, v in w.items()}
        latent, hidden = a["fc1_w"].shape[1], a["fc1_w"].shape[0]
        capi.check(self._lib.sfx_model_set_vposer(self._h, latent, hidden, capi.fptr(a["fc1_w"]), capi.fptr(a["fc1_b"]),
                                                  capi.fptr(a["fc2_w"]), capi.fptr(a["fc2_b"]),
                                                  capi.fptr(a["out_w"]), capi.fptr(a["out_b"])))
        self.vposer_latent = latent
        self.vposer_weights = a          # the encoder (if present) runs on the host: vposer.encode

    # the nine inputs of lbs_forward / lbs_backward under the reference's parameter names, in the C ABI's order
    LBS_INPUTS = ("global_orient", "body_pose", "betas", "expression", "jaw_pose", "leye_pose", "reye_pose",
                  "left_hand_pose", "right_hand_pose")

    @staticmethod
    def _lbs_arg(name, t, shape, dev, optional):
        """One tensor of lbs_forward / lbs_backward as the library reads it: float32, contiguous, of `shape`, on `dev` (any
        dtype is converted; a tensor elsewhere is moved there)."""
        import torch
        if torch.is_tensor(t):
            t = t.detach().to(dev)
            if name == "body_pose" and t.dim() != 2:      # [B][21][3] as the reference passes it
                t = t.reshape(shape[0], -1)
        return A.tensor(name, t, shape, dev, optional=optional, convert=True, make_contiguous=True, non_tensor=ValueError)

    def _lbs_inputs(self, ins, optional):
        """B, device (both global_orient's) and the nine inputs as [B][n] tensors; optional: None passes (a NULL pointer)."""
        B, dev = ins[0].shape[0], ins[0].device
        want = (3, 63, self.num_betas, self.num_expr, 3, 3, 3, self.num_pca, self.num_pca)
        return B, dev, [self._lbs_arg(name, t, (B, n), dev, optional) for name, t, n in zip(self.LBS_INPUTS, ins, want)]

    def lbs_forward(self, global_orient, body_pose, betas, expression, jaw_pose, leye_pose, reye_pose,
                    left_hand_pose, right_hand_pose, return_verts=True, return_full_pose=True, stream=None):
        """torch CUDA tensors in/out (containers only); one dense LBS launch sequence.  Inputs [B][n] of any dtype (body_pose
        [B][63] or [B][21][3]); None = not given."""
        import torch
        B, dev, ins = self._lbs_inputs((global_orient, body_pose, betas, expression, jaw_pose, leye_pose, reye_pose,
                                        left_hand_pose, right_hand_pose), optional=True)
        verts = torch.empty([B, self.V, 3], dtype=torch.float32, device=dev) if return_verts else None
        joints = torch.empty([B, self.K, 3], dtype=torch.float32, device=dev)
        fp = torch.empty([B, 165], dtype=torch.float32, device=dev) if return_full_pose else None
        capi.check(self._lib.sfx_lbs_forward(self._h, B, *[A.ptr(t) for t in ins + [verts, joints, fp]], A.stream(stream)))
        return verts, joints, fp

    def lbs_backward(self, global_orient, body_pose, betas, expression, jaw_pose, leye_pose, reye_pose,
                     left_hand_pose, right_hand_pose, dvertices=None, djoints=None, stream=None):
        """Gradient of sum(dvertices * vertices) + sum(djoints * joints) with respect to the nine inputs of lbs_forward
        (sfx_lbs_backward: what autograd through smplx.SMPLX.forward returns in the reference's ecosystem).  Stateless: the
        inputs are given again and the forward is re-evaluated at them.  dvertices [B][V][3] / djoints [B][K][3] are torch CUDA
        tensors, either may be None (joints only: no GEMM runs), not both.  Returns {name: float32 CUDA tensor} keyed by the
        reference's parameter names (LBS_INPUTS)."""
        import torch
        if dvertices is None and djoints is None:
            raise ValueError("lbs_backward needs an upstream gradient: dvertices, djoints or both")
        B, dev, ins = self._lbs_inputs((global_orient, body_pose, betas, expression, jaw_pose, leye_pose, reye_pose,
                                        left_hand_pose, right_hand_pose), optional=False)
        ups = [self._lbs_arg("dvertices", dvertices, (B, self.V, 3), dev, True),
               self._lbs_arg("djoints", djoints, (B, self.K, 3), dev, True)]
        outs = [torch.empty_like(t) for t in ins]
        capi.check(self._lib.sfx_lbs_backward(self._h, B, *[A.ptr(t) for t in ins + ups + outs], A.stream(stream)))
        return dict(zip(self.LBS_INPUTS, outs))


# an input of the stand-alone VPoser calls: any dtype and any strides are taken (converted, copied)
_vposer_in = functools.partial(A.tensor, convert=True, make_contiguous=True, non_tensor=ValueError)


def _flat(t):
    """[B][21][3] / [B][1][21][3], as the reference passes poses, -> [B][63]; anything else as it is."""
    import torch
    return t.reshape(t.shape[0], -1) if torch.is_tensor(t) and t.dim() > 2 else t


def _cuda(index):
    import torch
    return torch.device("cuda", index)


class VPoserDecoder(capi.Handle):
    """VPoser-v1 decoder weights resident in HBM (sfx_vposer): `decode` / `decode_backward` for whole batches of latents,
    outside any fit (inside one the closure workgroup decodes: csrc/vposer.h).  `weights` is the numpy dict
    DeviceModel.set_vposer takes (fc1_w [512][L], fc1_b, fc2_w, fc2_b, out_w [126][512], out_b).  The handle lives on the
    device that is current when it is made (`device_index`)."""
    _destroy = "sfx_vposer_destroy"

    def __init__(self, weights):
        lib = capi.load()
        a = {k: capi.f32(weights[k]) for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "out_w", "out_b")}
        hidden, latent = (int(n) for n in a["fc1_w"].shape)
        want = dict(fc1_b=(hidden,), fc2_w=(hidden, hidden), fc2_b=(hidden,), out_w=(126, hidden), out_b=(126,))
        for k, shape in want.items():
            if tuple(a[k].shape) != shape:
                raise ValueError("%s: shape %s, expected %s" % (k, tuple(a[k].shape), shape))
        h = C.c_void_p()
        capi.check(lib.sfx_vposer_create(latent, hidden, capi.fptr(a["fc1_w"]), capi.fptr(a["fc1_b"]), capi.fptr(a["fc2_w"]),
                                         capi.fptr(a["fc2_b"]), capi.fptr(a["out_w"]), capi.fptr(a["out_b"]), C.byref(h)))
        import torch
        self._h, self._lib = h, lib
        self.latent = latent
        self.device_index = torch.cuda.current_device()      # where the weights live: every tensor of a call must be there

    def decode(self, z, out=None, stream=None):
        """z [B][latent] (torch CUDA tensor) -> body_pose [B][63], axis-angle of the 21 body joints.  `out`: a float32
        contiguous [B][63] tensor on z's device to write into.  Only enqueues on the current (or the given) stream."""
        z = _vposer_in("z", z, (None, self.latent), _cuda(self.device_index), holder="the decoder's weights")
        B = z.shape[0]
        out = A.out_tensor("out", out, (B, 63), z.device)
        capi.check(self._lib.sfx_vposer_decode(self._h, B, A.ptr(z), A.ptr(out), A.stream(stream, z.device)))
        return out

    def decode_backward(self, z, dbody, out=None, stream=None):
        """d sum(dbody * decode(z)) / d z: [B][latent].  Stateless: z is given again and the forward re-evaluated at it."""
        z = _vposer_in("z", z, (None, self.latent), _cuda(self.device_index), holder="the decoder's weights")
        B = z.shape[0]
        dbody = _vposer_in("dbody", _flat(dbody), (B, 63), z.device, holder="z")
        out = A.out_tensor("out", out, (B, self.latent), z.device)
        capi.check(self._lib.sfx_vposer_decode_backward(self._h, B, A.ptr(z), A.ptr(dbody), A.ptr(out), A.stream(stream, z.device)))
        return out


_ENC_KEYS = ("enc_bn1_w", "enc_bn1_b", "enc_bn1_mean", "enc_bn1_var", "enc_fc1_w", "enc_fc1_b",
             "enc_bn2_w", "enc_bn2_b", "enc_bn2_mean", "enc_bn2_var", "enc_fc2_w", "enc_fc2_b",
             "enc_mu_w", "enc_mu_b", "enc_logvar_w", "enc_logvar_b")


class VPoserEncoder(capi.Handle):
    """VPoser-v1 encoder weights resident in HBM (sfx_vposer_encoder): `encode` / `encode_backward` for whole batches of
    poses.  `weights` is the numpy dict of vposer.load_vposer with its `enc_*` keys (bn1, fc1 [512][63 | 189], bn2, fc2, mu and
    logvar [L][512]); the batch norms are folded into the linear layers on the host.  The handle lives on the device that is
    current when it is made."""
    _destroy = "sfx_vposer_encoder_destroy"

    def __init__(self, weights):
        lib = capi.load()
        missing = [k for k in _ENC_KEYS if k not in weights]
        if missing:
            raise ValueError("these VPoser weights carry no encoder (bodyprior_enc_*): missing %s" % missing)
        a = {k: capi.f32(weights[k]) for k in _ENC_KEYS}
        if a["enc_fc1_w"].ndim != 2 or a["enc_mu_w"].ndim != 2:
            raise ValueError("enc_fc1_w / enc_mu_w: two-dimensional [out][in] arrays are needed")
        hidden, n_in = (int(n) for n in a["enc_fc1_w"].shape)
        latent = int(a["enc_mu_w"].shape[0])
        want = dict(enc_bn1_w=(n_in,), enc_bn1_b=(n_in,), enc_bn1_mean=(n_in,), enc_bn1_var=(n_in,), enc_fc1_b=(hidden,),
                    enc_bn2_w=(hidden,), enc_bn2_b=(hidden,), enc_bn2_mean=(hidden,), enc_bn2_var=(hidden,),
                    enc_fc2_w=(hidden, hidden), enc_fc2_b=(hidden,), enc_mu_w=(latent, hidden), enc_mu_b=(latent,),
                    enc_logvar_w=(latent, hidden), enc_logvar_b=(latent,))
        for k, shape in want.items():
            if tuple(a[k].shape) != shape:
                raise ValueError("%s: shape %s, expected %s" % (k, tuple(a[k].shape), shape))
        h = C.c_void_p()
        capi.check(lib.sfx_vposer_encoder_create(latent, hidden, n_in, *[capi.fptr(a[k]) for k in _ENC_KEYS], C.byref(h)))
        import torch
        self._h, self._lib = h, lib
        self.latent, self.n_in = latent, n_in
        self.device_index = torch.cuda.current_device()      # where the weights live: every tensor of a call must be there

    def _pose(self, pose):
        return _vposer_in("pose", _flat(pose), (None, 63), _cuda(self.device_index), holder="the encoder's weights")

    def encode(self, pose, out_mean=None, out_sigma=None, stream=None):
        """pose [B][63] (torch CUDA tensor; [B][21][3] and [B][1][21][3] are flattened) -> (mean, sigma), both [B][latent]: the
        two parameters of the Normal `vposer.encode(pose)` returns in the reference.  `out_mean` / `out_sigma`: float32
        contiguous [B][latent] tensors on pose's device to write into.  `out_sigma=False`: sigma is not wanted (a prior on the
        mean alone) -- it is neither evaluated nor stored, and (mean, None) is returned.  Only enqueues on the current (or the
        given) stream."""
        pose = self._pose(pose)
        B = pose.shape[0]
        mean = A.out_tensor("out_mean", out_mean, (B, self.latent), pose.device)
        sigma = None if out_sigma is False else A.out_tensor("out_sigma", out_sigma, (B, self.latent), pose.device)
        capi.check(self._lib.sfx_vposer_encode(self._h, B, A.ptr(pose), A.ptr(mean), A.ptr(sigma), A.stream(stream, pose.device)))
        return mean, sigma

    def encode_backward(self, pose, dmean, dsigma, out=None, stream=None):
        """d (sum(dmean * mean) + sum(dsigma * sigma)) / d pose: [B][63].  One of dmean / dsigma may be None (= zeros).
        Stateless: pose is given again and the forward re-evaluated at it."""
        pose = self._pose(pose)
        B = pose.shape[0]
        if dmean is None and dsigma is None:
            raise ValueError("dmean and dsigma: at least one is needed")
        grads = [_vposer_in(name, d, (B, self.latent), pose.device, optional=True, holder="pose")
                 for name, d in (("dmean", dmean), ("dsigma", dsigma))]
        out = A.out_tensor("out", out, (B, 63), pose.device)
        capi.check(self._lib.sfx_vposer_encode_backward(self._h, B, A.ptr(pose), A.ptr(grads[0]), A.ptr(grads[1]), A.ptr(out),
                                                        A.stream(stream, pose.device)))
        return out


PRECISIONS = ("mixed", "float64")


def check_precision(cfg, lbs_mode="rows", has_regression_pose=True, precision="mixed"):
    """sfx_batch_cfg.high_precision of a FrameBatch (include/sfx.h):
      "mixed" (default): cfg float_dtype picks 0 (float32) or 1 (float64: fp64 projection, fp32 parameters and reverse sweep);
      "float64": 2, the closure in float64 -- the body-only needed-rows path, and only with float_dtype: float64.  An engine-level
      option of FrameBatch (closure / last_grad): the device optimiser is fp32, so the driver and main never select it.
    Raises ValueError naming the setting the float64 mode does not support (what sfx_batch_create would refuse)."""
    precision = str(precision or "mixed")
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s, got %r" % (", ".join(PRECISIONS), precision))
    float64 = str(cfg.get("float_dtype", "float32")) == "float64"
    if precision == "mixed":
        return int(float64 or bool(cfg.get("high_precision", False)))
    unsupported = [("float_dtype: %s (precision: float64 needs float_dtype: float64)" % cfg.get("float_dtype", "float32"), not float64),
                   ("lbs_mode=%r (needs 'rows')" % lbs_mode, lbs_mode != "rows"),
                   ("use_vposer", bool(cfg.get("use_vposer", True))),
                   ("use_hands", bool(cfg.get("use_hands", True))),
                   ("use_face", bool(cfg.get("use_face", True))),
                   ("interpenetration", bool(cfg.get("interpenetration", False))),
                   ("the GMM body pose prior (no regression pose)", not has_regression_pose and not cfg.get("use_vposer", True))]
    bad = [name for name, hit in unsupported if hit]
    if bad:
        raise ValueError("precision: float64 does not support %s" % "; ".join(bad))
    return 2


def widen_stage_weights(stages):
    """capi.StageWeights -> capi.StageWeights64 (the float values widened)."""
    out = []
    for w in stages:
        d = capi.StageWeights64()
        for name, _ in capi.StageWeights._fields_:
            if name == "jaw_prior_weight":
                for q in range(3):
                    d.jaw_prior_weight[q] = w.jaw_prior_weight[q]
            else:
                setattr(d, name, getattr(w, name))
        out.append(d)
    return out


# the two number formats a FrameBatch exchanges its host arrays in: numpy dtype, conversion to it (contiguous), pointer,
# suffix of the sfx_batch_* entry points that take it
_Mode = collections.namedtuple("_Mode", "dtype cast ptr suffix")
_F32 = _Mode(np.float32, capi.f32, capi.fptr, "")
_F64 = _Mode(np.float64, capi.f64, capi.dptr, "_f64")


def _focal_pairs(focal, B, dtype):
    """[B][2] = (fx, fy) of every frame from `focal`: a number or [B] (fx = fy), or [B, 2] = (fx, fy) per frame."""
    f = np.asarray(focal, dtype)
    if f.ndim == 0 or f.shape == (B,):
        return np.broadcast_to(f.reshape(-1, 1), (B, 2))
    if f.shape == (B, 2):
        return f
    raise ValueError("focal must be a number, [B] or [B, 2] = (fx, fy) with B = %d, got shape %r" % (B, tuple(f.shape)))


def _pack_frames(m, B, K, keypoints, joint_weights, cam_init_mask, focal, center, data_weight, est_tz=None, cam_rot=None):
    """The five arrays of sfx_batch_set_frames in mode `m`: keypoints [B][K][3], joint weights and camera-init mask [B][K] (one
    frame's are broadcast), the camera record [B][6] = (fx, fy, cx, cy, data_weight, est_tz or 0) and the rotation [B][9]
    (None = identity).  `focal`: a number or [B] (fx = fy), or [B, 2] = (fx, fy).  The data -- keypoints, weights, masks,
    rotation -- are fp32 numbers, widened in float64 mode; the camera record is made in the mode's own dtype."""
    kp = m.cast(capi.f32(keypoints)).reshape(B, K, 3)
    jw = m.cast(np.broadcast_to(np.asarray(joint_weights, np.float32), (B, K)))
    cm = m.cast(np.broadcast_to(np.asarray(cam_init_mask, np.float32), (B, K)))
    cam = np.zeros((B, 6), m.dtype)
    cam[:, 0:2] = _focal_pairs(focal, B, m.dtype)
    cam[:, 2:4] = np.asarray(center, m.dtype).reshape(-1, 2)
    cam[:, 4] = np.asarray(data_weight, m.dtype)
    if est_tz is not None:
        cam[:, 5] = np.asarray(est_tz, m.dtype)
    R = np.tile(np.eye(3, dtype=m.dtype).reshape(1, 9), (B, 1)) if cam_rot is None else capi.f32(cam_rot).reshape(B, 9)
    return kp, jw, cm, cam, m.cast(R)


def _pack_params(m, B, sizes, nemb, regression_pose, params):
    """The arguments of sfx_batch_set_params in mode `m`: one [B][sizes[name]] array (one frame's values are broadcast) or
    None per PARAM_NAMES entry, taken in the mode's own dtype, and the regression pose [B][nemb], an fp32 number in both."""
    args = [None if params.get(n) is None else
            m.cast(np.broadcast_to(np.asarray(params[n], m.dtype).reshape(-1, sizes[n]), (B, sizes[n]))) for n in PARAM_NAMES]
    reg = None if regression_pose is None else m.cast(capi.f32(
        np.broadcast_to(np.asarray(regression_pose, np.float32).reshape(-1, nemb), (B, nemb))))
    return args, reg


class FrameBatch(capi.Handle):
    """B frames under one configuration (sfx_batch)."""
    _destroy = "sfx_batch_destroy"

    def __init__(self, model, B, cfg, lbs_mode="dense", reuse_entry_eval=True, has_regression_pose=True,
                 stages=None, num_body_joints=None, side_view=False, slots=0, precision="mixed"):
        """`cfg` uses the reference's key names (cmd_parser).  `stages` (list of
        capi.StageWeights) overrides the schedule derived from cfg; `num_body_joints` overrides
        where the per-stage hand/face joint weights start (K = never: weights passed verbatim).
        `slots` (dense mode): GEMM columns when B is larger -- the other frames queue and are admitted as
        columns free up (continuous batching); 0 = one column per frame.
        `precision`: "mixed" (default; cfg float_dtype picks the mode as always) or "float64", a float64 batch
        (check_precision): every real number it takes and returns is float64, and it evaluates closures (closure / last_grad)
        only -- fit, step, guess_init, stats and trace are fp32-only and refused."""
        self.model, self.B, self.cfg = model, int(B), dict(cfg)
        self._lib = model._lib
        hp = check_precision(cfg, lbs_mode, has_regression_pose, precision)
        self.float64 = hp == 2
        self._mode = _F64 if self.float64 else _F32
        stages64 = None
        if self.float64:
            stages64 = stage_weights_from_cfg(cfg, capi.StageWeights64)[0] if stages is None else widen_stage_weights(stages)
        if stages is None:
            stages, _ = stage_weights_from_cfg(cfg)
        self.n_stages = len(stages)
        c = capi.BatchCfg()
        c.B = self.B
        c.n_stages = self.n_stages
        c.use_vposer = int(bool(cfg.get("use_vposer", True)))
        c.use_hands = int(bool(cfg.get("use_hands", True)))
        c.use_face = int(bool(cfg.get("use_face", True)))
        c.use_joints_conf = int(bool(cfg.get("use_joints_conf", False)))
        c.has_regression_pose = int(bool(has_regression_pose))
        c.use_conf_cam_init = int(bool(cfg.get("use_conf_for_camera_init", False)))
        c.num_body_joints = (NUM_BODY_JOINTS[cfg.get("format", "coco25")] if num_body_joints is None
                             else int(num_body_joints))
        c.maxiters = int(cfg.get("maxiters", 30))
        c.ftol = float(cfg.get("ftol", 1e-9)); c.gtol = float(cfg.get("gtol", 1e-9))
        c.lr = float(cfg.get("lr", 1.0)); c.rho = float(cfg.get("rho", 100))
        c.depth_loss_weight = float(cfg.get("depth_loss_weight", 1e2))
        c.lbs_mode = {"rows": 0, "dense": 1}[lbs_mode]
        c.reuse_entry_eval = int(bool(reuse_entry_eval))
        c.side_view_thsh = float(cfg.get("side_view_thsh", 0.0) or 0.0) if side_view else 0.0
        c.left_shoulder_idx = int(cfg.get("left_shoulder_idx", 2))
        c.right_shoulder_idx = int(cfg.get("right_shoulder_idx", 5))
        # interpenetration term (fitting.py:437-455): dense mode only, part labels from DeviceModel.set_parts
        c.interpenetration = int(bool(cfg.get("interpenetration", False)))
        c.max_collisions = int(cfg.get("max_collisions", 8))
        c.df_cone_height = float(cfg.get("df_cone_height", 0.5))
        c.penalize_outside = int(bool(cfg.get("penalize_outside", True)))
        c.point2plane = int(bool(cfg.get("point2plane", False)))
        if c.point2plane and cfg.get("interpenetration", False):
            _warn_point2plane()
        c.slots = int(slots or 0)
        # LBFGS hyper-parameters (optimizers/lbfgs_ls.py); the cfg files never set them: 0 = the reference's defaults
        # (tolerances: negative = default; an explicit 0 -- LBFGS(tolerance_grad=0): the test is disabled -- is passed through)
        tg, tc = cfg.get("lbfgs_tolerance_grad"), cfg.get("lbfgs_tolerance_change")
        c.lbfgs_tolerance_grad = -1.0 if tg is None else float(tg)
        c.lbfgs_tolerance_change = -1.0 if tc is None else float(tc)
        c.lbfgs_max_eval = int(cfg.get("lbfgs_max_eval", 0) or 0)
        c.lbfgs_history_size = int(cfg.get("lbfgs_history_size", 0) or 0)
        c.lbfgs_max_iter = int(cfg.get("lbfgs_max_iter", 0) or 0)
        # cfg float_dtype: float64 (main.py:99-105) -> the engine's high-precision mode (include/sfx.h sfx_batch_cfg.high_precision);
        # precision="float64" -> mode 2
        c.high_precision = hp
        if c.interpenetration and lbs_mode != "dense":
            raise ValueError("interpenetration=True needs lbs_mode='dense' (the term reads every vertex)")
        self.use_vposer = bool(c.use_vposer)
        self.nemb = model.vposer_latent if self.use_vposer else 63
        arr = (capi.StageWeights * max(1, self.n_stages))(*stages)
        h = C.c_void_p()
        capi.check(self._lib.sfx_batch_create(model._h, C.byref(c), arr, C.byref(h)))
        self._h = h
        self.K = model.K
        self._trace_cap = 0
        if self.float64:
            arr64 = (capi.StageWeights64 * max(1, self.n_stages))(*stages64)
            capi.check(self._lib.sfx_batch_set_stage_weights_f64(self._h, arr64))

    # ---- data ------------------------------------------------------------------------------
    def _call(self, name, *args):
        """sfx_batch_<name> in the batch's own number format (_Mode.suffix)."""
        capi.check(getattr(self._lib, "sfx_batch_" + name + self._mode.suffix)(self._h, *args))

    def set_frames(self, keypoints, joint_weights, cam_init_mask, focal, center, data_weight, est_tz=None,
                   cam_rot=None):
        """Per-frame data (_pack_frames).  focal: a number or [B] (fx = fy), or [B, 2] = (fx, fy) per frame; center [B, 2];
        data_weight and est_tz a number or [B]; cam_rot [B, 3, 3] row-major (None: identity)."""
        arrays = _pack_frames(self._mode, self.B, self.K, keypoints, joint_weights, cam_init_mask, focal, center, data_weight,
                              est_tz, cam_rot)
        self._call("set_frames", *[self._mode.ptr(a) for a in arrays])

    def _sizes(self):
        return dict(cam_translation=3, global_orient=3, betas=self.model.num_betas,
                    left_hand_pose=self.model.num_pca, right_hand_pose=self.model.num_pca,
                    expression=self.model.num_expr, jaw_pose=3, leye_pose=3, reye_pose=3,
                    pose_embedding=self.nemb)

    def set_params(self, regression_pose=None, **p):
        args, reg = _pack_params(self._mode, self.B, self._sizes(), self.nemb, regression_pose, p)
        self._call("set_params", *[self._mode.ptr(a) for a in args + [reg]])

    def get_params(self):
        sizes = self._sizes()
        outs = [np.zeros((self.B, n), self._mode.dtype) for n in [sizes[name] for name in PARAM_NAMES] + [63]]
        self._call("get_params", *[self._mode.ptr(a) for a in outs])
        return dict(zip(PARAM_NAMES + ("body_pose",), outs))

    # ---- compute ---------------------------------------------------------------------------
    def num_vars(self, stage):
        return self._lib.sfx_batch_num_vars(self._h, stage)

    def closure(self, stage):
        """(loss[B], grad[B,N]) at the current parameters; stage -1 = camera-init loss.  float64 on a float64 batch."""
        m = self._mode
        loss = np.zeros(self.B, m.dtype)
        grad = np.zeros((self.B, self.num_vars(stage)), m.dtype)
        self._call("closure", stage, m.ptr(loss), m.ptr(grad), None)
        return loss, grad

    def guess_init(self, pairs):
        p = capi.i32(np.asarray(pairs).reshape(-1, 2))
        capi.check(self._lib.sfx_batch_guess_init(self._h, capi.iptr(p), p.shape[0], None))

    def fit(self, first_stage=-1, last_stage=None, stream=None):
        last = self.n_stages - 1 if last_stage is None else last_stage
        capi.check(self._lib.sfx_batch_fit(self._h, first_stage, last, C.c_void_p(stream) if stream else None))

    def step(self, stage, resume):
        """One LBFGS.step for every frame; returns the entry losses [B]."""
        loss = np.zeros(self.B, np.float32)
        capi.check(self._lib.sfx_batch_step(self._h, stage, int(bool(resume)), capi.fptr(loss), None))
        return loss

    def set_gmm(self, prior):
        """Body pose prior = prior.MaxMixturePrior (body_prior_type 'gmm'): used by the closure when
        use_vposer is off and the batch has no regression pose (fitting.py:399-401)."""
        mu = np.ascontiguousarray(prior.means.detach().cpu().numpy(), np.float32)
        P = np.ascontiguousarray(prior.precisions.detach().cpu().numpy(), np.float32)
        nw = np.ascontiguousarray(prior.nll_weights.detach().cpu().numpy().reshape(-1), np.float32)
        # MaxMixturePrior.log_likelihood (prior.py:203-225): d^T P d + 0.5 (log(det cov + eps) + D log 2 pi) per component
        cc = prior.component_constants() if hasattr(prior, "component_constants") else None
        if cc is not None:
            cc = np.ascontiguousarray(cc.detach().cpu().numpy().reshape(-1), np.float32)
        capi.check(self._lib.sfx_batch_set_gmm_form(self._h, mu.shape[0], mu.shape[1], capi.fptr(mu), capi.fptr(P), capi.fptr(nw),
                                                    capi.fptr(cc) if cc is not None else None))

    _DEBUG_PER_FRAME = dict(verts="V3", vposed="V3", pen_dverts="V3", pen_dfeat=512, feat=512, pen_dA=55 * 12, A=12 * 55,
                            pen_loss=1, uvp="U3", uvp_self="U3")

    def debug_read(self, name):
        """Tests: one of the dense path's device buffers of the most recent evaluation as [B, per-frame]
        (sfx_batch_debug_read)."""
        per = self._DEBUG_PER_FRAME[name]
        per = self.model.V * 3 if per == "V3" else (self.model.n_uniq * 3 if per == "U3" else per)
        out = np.zeros((self.B, per), np.float32)
        if per == 0:            # (a model whose keypoints are all kinematic joints exports no vertex: nothing to copy or launch)
            return out
        capi.check(self._lib.sfx_batch_debug_read(self._h, name.encode(), capi.fptr(out), out.size))
        return out

    def penetration_stats(self):
        """Diagnostics of the interpenetration term of the most recent evaluation (per frame):
        ordered pairs kept, partners dropped by max_collisions, grid overflow, vertices with gradient."""
        st = np.zeros((self.B, 4), np.int32)
        ext = np.zeros(self.B, np.int32)
        capi.check(self._lib.sfx_batch_pen_stats(self._h, capi.iptr(st), capi.iptr(ext)))
        return dict(pairs=st[:, 0].copy(), dropped=st[:, 1].copy(), entry_overflow=st[:, 2].copy(), walks_cut=st[:, 3].copy(), vertices=ext)

    def penetration_pairs(self, column):
        """Ordered pair list [n, 2] (receiving triangle, partner) of GEMM column `column` in the most recent evaluation
        (sfx_batch_pen_pairs): what BVH + FilterFaces hand to the loss in the reference (fitting.py:445-450)."""
        return _read_pairs(lambda cap, buf, n: self._lib.sfx_batch_pen_pairs(self._h, int(column), cap, buf, n))

    def penetration_flags(self):
        """Per frame: True when the frame's fit consumed a collision evaluation whose pair set depended on arrival order
        (a cut bucket walk; with max_collisions > 1024 also a partner list beyond 2 x max_collisions): its result is not
        reproducible run to run."""
        fl = np.zeros(self.B, np.int32)
        capi.check(self._lib.sfx_batch_pen_flags(self._h, capi.iptr(fl)))
        return fl != 0

    def penetration_launches(self):
        """Kernel launches of one interpenetration step of the fitting loop, counted on the captured graph (0 before a fit)."""
        return int(self._lib.sfx_batch_pen_launches(self._h))

    def last_grad(self, stage):
        """Gradient [B,N] of the most recent closure evaluation (what var.grad holds after step()); float64 on a float64 batch."""
        grad = np.zeros((self.B, self.num_vars(stage)), self._mode.dtype)
        self._call("get_grad", stage, self._mode.ptr(grad))
        return grad

    def trace(self, capacity, evaluations=False):
        """Attach (capacity > 0 records per frame) or detach (0) the optimiser trace (sfx_batch_trace);
        evaluations=True adds one record per closure evaluation."""
        capi.check(self._lib.sfx_batch_trace(self._h, -int(capacity) if evaluations else int(capacity)))
        self._trace_cap = int(capacity)

    def get_trace(self):
        """Per frame: array [n, 4] of the records written since the trace was attached
        ((0, t, loss, ls_evals) | (1, entry loss, func_evals, n_iter) | (2, result, evals, stage))."""
        cap = self._trace_cap
        rec = np.zeros((self.B, cap, 4), np.float32)
        cnt = np.zeros(self.B, np.int32)
        capi.check(self._lib.sfx_batch_get_trace(self._h, capi.fptr(rec), capi.iptr(cnt)))
        if (cnt > cap).any():
            raise RuntimeError("optimiser trace overflowed: %d records, capacity %d" % (cnt.max(), cap))
        return [rec[i, :cnt[i]].copy() for i in range(self.B)]

    def stats(self):
        ns = self.n_stages + 1
        loss = np.zeros((self.B, ns), np.float32)
        ev = np.zeros((self.B, ns), np.int32)
        rev = np.zeros((self.B, ns), np.int32)
        capi.check(self._lib.sfx_batch_get_stats(self._h, capi.fptr(loss), capi.iptr(ev), capi.iptr(rev)))
        return dict(stage_loss=loss, stage_evals=ev, stage_ref_evals=rev)

    def forward(self, want_verts=True):
        """Final meshes/joints at the current parameters as torch CUDA tensors."""
        import torch
        dev = _cuda(torch.cuda.current_device())
        verts = torch.empty([self.B, self.model.V, 3], dtype=torch.float32, device=dev) if want_verts else None
        joints = torch.empty([self.B, self.K, 3], dtype=torch.float32, device=dev)
        capi.check(self._lib.sfx_batch_forward(self._h, A.ptr(verts), A.ptr(joints), None))
        return verts, joints


class BatchOptimizer(capi.Handle):
    """The engine's optimiser for losses the CALLER evaluates (sfx_opt_*, csrc/opt_ext.hip): B independent problems of N <= 192
    float32 variables, each with its own run_fitting / LBFGS.step / strong-Wolfe state on the device (one wavefront per problem,
    one evaluation of every running problem per launch).  Reverse communication over torch CUDA tensors:

        opt.begin(x0)                        # [B][N]; opt.x_trial [B][N] now holds the first points to evaluate
        while opt.active():                  # the loop's only host synchronisation (4 bytes)
            loss, grad = evaluate(opt.x_trial)      # [B], [B][N], by any means: the device never sees the objective
            opt.tell(loss, grad)             # opt.x_trial holds the next points; rows of finished problems stay put
        r = opt.result()

    groups: lengths of the tensors the N variables are made of (run_fitting's gtol test looks at each tensor's gradient,
    fitting.py:191); None = one tensor.  Hyper-parameters: maxiters, ftol, gtol (FittingMonitor), lr, max_iter, max_eval,
    history_size, tolerance_grad, tolerance_change (lbfgs_ls.LBFGS; defaults of oracle/lbfgs_machine.StageMachine, whose
    spellings history / tol_grad / tol_change are accepted too), reuse_entry_eval.  There is no CPU fallback."""

    _PREFIX = "sfx_opt_"                    # the handle's symbols: _PREFIX + create / begin / tell / active / get / trace / get_trace
    _destroy = "sfx_opt_destroy"
    _ALIASES = dict(history="history_size", tol_grad="tolerance_grad", tol_change="tolerance_change")
    _STATE = "the optimiser's state"        # what lives on self.device, for the message that refuses a tensor elsewhere

    def __init__(self, B, N, groups=None, **hyper):
        h = dict(maxiters=30, ftol=1e-9, gtol=1e-9, lr=1.0, max_iter=None, max_eval=None, history_size=100,
                 tolerance_grad=1e-5, tolerance_change=1e-9, reuse_entry_eval=False)
        for k, v in hyper.items():
            k = self._ALIASES.get(k, k)
            if k not in h:
                raise TypeError("%s: unknown hyper-parameter %r (known: %s)" % (type(self).__name__, k, ", ".join(sorted(h))))
            h[k] = v
        lib = capi.load()
        groups = [int(n) for n in groups] if groups is not None else []
        c = self._cfg(groups)
        c.B, c.N, c.n_groups = int(B), int(N), len(groups)
        c.maxiters, c.ftol, c.gtol, c.lr = int(h["maxiters"]), float(h["ftol"]), float(h["gtol"]), float(h["lr"])
        c.tolerance_grad, c.tolerance_change = float(h["tolerance_grad"]), float(h["tolerance_change"])
        c.max_iter = int(h["max_iter"]) if h["max_iter"] is not None else 0
        c.max_eval = int(h["max_eval"]) if h["max_eval"] is not None else 0
        if c.max_iter < 0 or c.max_eval < 0 or (h["max_iter"] is not None and c.max_iter == 0) or (h["max_eval"] is not None and c.max_eval == 0):
            raise ValueError("%s: max_iter / max_eval must be positive (None = the reference's defaults)" % type(self).__name__)
        c.history_size = int(h["history_size"]) if int(h["history_size"]) >= 1 else -1      # (0 is the C structure's "default": not offered here)
        c.reuse_entry_eval = int(bool(h["reuse_entry_eval"]))
        hnd = C.c_void_p()
        capi.check(getattr(lib, self._PREFIX + "create")(C.byref(c), C.byref(hnd)))
        import torch
        self._h, self._lib = hnd, lib
        self.B, self.N, self.hyper = int(B), int(N), h
        self.device = _cuda(torch.cuda.current_device())      # where the state lives: every tensor of a call must be there
        self.x_trial = None
        self._trace_cap = 0

    @staticmethod
    def _cfg(groups):
        """The configuration structure with the tensors' lengths in place."""
        c = capi.OptCfg()
        for i, n in enumerate(groups[:12]):      # (a longer list is refused by the library through n_groups)
            c.group_len[i] = n
        return c

    def _call(self, name, *args):
        capi.check(getattr(self._lib, self._PREFIX + name)(self._h, *args))

    def begin(self, x0, mode="fit", resume=False, stream=None):
        """Start at x0 [B][N].  mode "fit": the whole run_fitting loop; "step": ONE LBFGS.step (resume=True continues the
        optimiser of the previous "step" run: history and counters kept).  Returns x_trial, the [B][N] tensor every later
        `tell` rewrites in place: the points to evaluate."""
        import torch
        if mode not in ("fit", "step"):
            raise ValueError("mode: 'fit' or 'step', got %r" % (mode,))
        x0 = A.tensor("x0", x0, (self.B, self.N), self.device, holder=self._STATE)
        if self.x_trial is None:
            self.x_trial = torch.empty((self.B, self.N), dtype=torch.float32, device=self.device)
        self._call("begin", 0 if mode == "fit" else 1, int(bool(resume)), A.ptr(x0), A.ptr(self.x_trial), A.stream(stream, self.device))
        return self.x_trial

    def tell(self, loss, grad, stream=None):
        """loss [B] and grad [B][N] at x_trial -> x_trial holds the next points.  Enqueues only.  Problems that have finished
        ignore their entries, so calling this more often than needed is harmless."""
        if self.x_trial is None:
            raise RuntimeError("%s.tell before begin" % type(self).__name__)
        loss = A.tensor("loss", loss, (self.B,), self.device, holder=self._STATE)
        grad = A.tensor("grad", grad, (self.B, self.N), self.device, holder=self._STATE)
        self._call("tell", A.ptr(loss), A.ptr(grad), A.ptr(self.x_trial), A.stream(stream, self.device))

    def active(self, stream=None):
        """Problems still running.  Waits for the stream: the one host synchronisation of a loop."""
        n = C.c_int32(0)
        self._call("active", C.byref(n), A.stream(stream, self.device))
        return int(n.value)

    def result(self):
        """dict: x [B][N] accepted points and grad [B][N] gradients of the last consumed evaluations (CUDA tensors); result [B]
        (mode "fit": what run_fitting returns, NaN for None; "step": the loss at entry), evals [B], status [B] (1 = finished)."""
        import torch
        x = torch.empty((self.B, self.N), dtype=torch.float32, device=self.device)
        g = torch.empty((self.B, self.N), dtype=torch.float32, device=self.device)
        res = np.zeros(self.B, np.float32)
        ev = np.zeros(self.B, np.int32)
        st = np.zeros(self.B, np.int32)
        self._call("get", A.ptr(x), A.ptr(g), capi.fptr(res), capi.iptr(ev), capi.iptr(st))
        return dict(x=x, grad=g, result=res, evals=ev, status=st)

    def trace(self, capacity):
        """Attach (capacity > 0 records per problem) or detach (0) the optimiser trace (sfx_opt_trace); a fresh begin empties it."""
        self._call("trace", int(capacity))
        self._trace_cap = int(capacity)

    def get_trace(self):
        """Per problem: array [n, 4] of the records of the current run
        ((0, t, loss, ls_evals) | (1, entry loss, func_evals, n_iter) | (2, result, evals, 0))."""
        cap = self._trace_cap
        rec = np.zeros((self.B, cap, 4), np.float32)
        cnt = np.zeros(self.B, np.int32)
        self._call("get_trace", capi.fptr(rec), capi.iptr(cnt))
        if (cnt > cap).any():
            raise RuntimeError("optimiser trace overflowed: %d records, capacity %d" % (cnt.max(), cap))
        return [rec[i, :cnt[i]].copy() for i in range(self.B)]


class WideOptimizer(BatchOptimizer):
    """BatchOptimizer for problems of up to 32768 variables in up to 256 tensors (sfx_opt_wide_*, csrc/opt_wide.hip): the same
    state machine on a vector layer one workgroup wide -- one workgroup of 1024 threads per problem, the working vectors and
    the history in device memory, dot products accumulated in float64.  The same methods, hyper-parameters and contracts; what
    a loss that couples frames needs (one shape over a clip, a temporal smoothness term, per-vertex offsets)."""

    _PREFIX = "sfx_opt_wide_"
    _destroy = "sfx_opt_wide_destroy"
    NMAX, MAX_GROUPS = 32768, 256           # SFX_WIDE_NMAX, SFX_WIDE_MAX_GROUPS

    @staticmethod
    def _cfg(groups):
        c = capi.OptWideCfg()
        c._lens = (C.c_int32 * max(1, len(groups)))(*groups)      # (read by sfx_opt_wide_create only; kept with the structure)
        c.group_len = C.cast(c._lens, C.POINTER(C.c_int32))
        return c


# ---- the objective on tensors the caller supplies (sfx_objective_eval / sfx_camera_init_eval, csrc/objective_ext.hip) --------
PRIOR_FORMS = dict(embedding=0, target=1, body_pose=2, mixture=3)      # SFX_PRIOR_*
OBJECTIVE_MAX_K = 512                                                   # keypoints per frame (OBJ_MAX_K)
OBJECTIVE_WEIGHTS = ("data_weight", "body_pose_weight", "shape_weight", "bending_prior_weight", "hand_prior_weight",
                     "expr_prior_weight")
# gradient names of objective_eval, in the order of sfx_objective_grads
OBJECTIVE_GRADS = ("joints", "rotation", "translation", "body_pose", "prior", "betas", "expression", "jaw_pose",
                   "left_hand_pose", "right_hand_pose")


def _obj_joints(joints):
    import torch
    if not torch.is_tensor(joints) or joints.dim() != 3 or joints.shape[2] != 3:
        raise ValueError("joints: shape %s, expected (B, K, 3)" % (tuple(getattr(joints, "shape", ())),))
    B, K = int(joints.shape[0]), int(joints.shape[1])
    if B < 1:
        raise ValueError("joints: at least one frame is needed, got B = %d" % B)
    if K < 1 or K > OBJECTIVE_MAX_K:
        raise ValueError("joints: K = %d keypoints, supported 1..%d" % (K, OBJECTIVE_MAX_K))
    return B, K, A.tensor("joints", joints, (B, K, 3))


def objective_eval(joints, rotation, translation, focal_x, focal_y, center, gt_joints, joint_weights, body_pose, prior, betas,
                   joints_conf=None, prior_target=None, expression=None, jaw_pose=None, left_hand_pose=None,
                   right_hand_pose=None, weights=None, jaw_prior_weight=(0.0, 0.0, 0.0), rho=100.0, use_joints_conf=True,
                   use_hands=True, use_face=True, prior_form="embedding", mixture=None, want_grads=True, stream=None):
    """SMPLifyLoss.forward (fitting.py:375-461, no interpenetration) and its gradient for B frames in one launch
    (sfx_objective_eval).  Every tensor is a float32 contiguous CUDA tensor: joints [B, K, 3], rotation [B, 3, 3],
    translation [B, 3], focal_x / focal_y [B], center [B, 2], gt_joints [B, K, 2], joints_conf / joint_weights [B, K],
    body_pose [B, 63] (the angle prior's operand), prior [B, n] (the pose prior's operand; prior_form 'embedding' | 'target' --
    with prior_target [B, n] -- | 'body_pose' | 'mixture' -- with mixture = dict(means [M, 63], precisions [M, 63, 63],
    nll_weights [M], comp_const [M] or None: CUDA tensors as prior.mixture_tables makes them)), betas, expression, jaw_pose
    [B, 3], left_hand_pose / right_hand_pose [B, 45].  weights: {name: float} over OBJECTIVE_WEIGHTS (missing = 0).
    Returns (loss [B], {name: gradient of loss[b] with respect to that input} over OBJECTIVE_GRADS) -- ({} when
    want_grads is off).  Only enqueues on the current (or the given) stream."""
    import torch
    B, K, joints = _obj_joints(joints)
    dev = joints.device
    arg = functools.partial(A.tensor, device=dev, optional=True, holder="joints")      # every other tensor: where joints is
    if prior_form not in PRIOR_FORMS:
        raise ValueError("prior_form: one of %s, got %r" % (sorted(PRIOR_FORMS), prior_form))
    if not torch.is_tensor(prior) or prior.dim() != 2:
        raise ValueError("prior: shape %s, expected (B, n)" % (tuple(getattr(prior, "shape", ())),))
    n = int(prior.shape[1])
    nb = int(betas.shape[1]) if torch.is_tensor(betas) and betas.dim() == 2 else -1
    ne = int(expression.shape[1]) if torch.is_tensor(expression) and expression.dim() == 2 else 0
    if use_joints_conf and joints_conf is None:
        raise ValueError("use_joints_conf needs joints_conf")
    if prior_form == "target" and prior_target is None:
        raise ValueError("prior_form 'target' needs prior_target")
    if use_hands and (left_hand_pose is None or right_hand_pose is None):
        raise ValueError("use_hands needs left_hand_pose and right_hand_pose")
    if use_face and (expression is None or jaw_pose is None):
        raise ValueError("use_face needs expression and jaw_pose")
    ins = dict(joints=joints,
               cam_rot=arg("rotation", rotation, (B, 3, 3)), cam_t=arg("translation", translation, (B, 3)),
               focal_x=arg("focal_x", focal_x, (B,)), focal_y=arg("focal_y", focal_y, (B,)),
               center=arg("center", center, (B, 2)), gt_joints=arg("gt_joints", gt_joints, (B, K, 2)),
               joints_conf=arg("joints_conf", joints_conf, (B, K)),
               joint_weights=arg("joint_weights", joint_weights, (B, K)),
               body_pose=arg("body_pose", body_pose, (B, 63)), prior=arg("prior", prior, (B, n)),
               prior_target=arg("prior_target", prior_target, (B, n)) if prior_form == "target" else None,
               betas=arg("betas", betas, (B, nb)),
               expression=arg("expression", expression, (B, ne)) if use_face else None,
               jaw=arg("jaw_pose", jaw_pose, (B, 3)) if use_face else None,
               lhand=arg("left_hand_pose", left_hand_pose, (B, 45)) if use_hands else None,
               rhand=arg("right_hand_pose", right_hand_pose, (B, 45)) if use_hands else None)
    c = capi.ObjectiveCfg()
    c.rho = float(rho)
    weights = weights or {}
    unknown = set(weights) - set(OBJECTIVE_WEIGHTS)
    if unknown:
        raise TypeError("objective_eval: unknown weights %s (known: %s)" % (sorted(unknown), ", ".join(OBJECTIVE_WEIGHTS)))
    for name in OBJECTIVE_WEIGHTS:
        setattr(c, name, float(weights.get(name, 0.0)))
    for q in range(3):
        c.jaw_prior_weight[q] = float(jaw_prior_weight[q])
    c.use_joints_conf, c.use_hands, c.use_face = int(bool(use_joints_conf)), int(bool(use_hands)), int(bool(use_face))
    c.prior_form = PRIOR_FORMS[prior_form]
    keep = []
    if prior_form == "mixture":
        if mixture is None:
            raise ValueError("prior_form 'mixture' needs the mixture's tables")
        mu = mixture["means"]
        if not torch.is_tensor(mu) or mu.dim() != 2:
            raise ValueError("mixture['means']: a [M, D] tensor is needed")
        M, D = int(mu.shape[0]), int(mu.shape[1])
        if D != 63 or n != 63:
            raise ValueError("the mixture prior acts on the 63 body-pose values: means [M, %d], operand [B, %d]" % (D, n))
        keep = [arg("mixture['means']", mu, (M, D)), arg("mixture['precisions']", mixture["precisions"], (M, D, D)),
                arg("mixture['nll_weights']", mixture["nll_weights"], (M,)),
                arg("mixture['comp_const']", mixture.get("comp_const"), (M,))]
        c.gmm_M, c.gmm_D = M, D
        c.gmm_means_dev, c.gmm_precisions_dev, c.gmm_nll_weights_dev, c.gmm_comp_const_dev = [t.data_ptr() if t is not None else None for t in keep]
    a = capi.ObjectiveIn()
    a.B, a.K, a.n_prior, a.num_betas, a.num_expr = B, K, n, nb, ne
    for name in capi.OBJECTIVE_INPUTS:
        setattr(a, name + "_dev", ins[name].data_ptr() if ins[name] is not None else None)
    loss = torch.empty([B], dtype=torch.float32, device=dev)
    grads, g = {}, None
    if want_grads:
        like = dict(joints=ins["joints"], rotation=ins["cam_rot"], translation=ins["cam_t"], body_pose=ins["body_pose"],
                    prior=ins["prior"], betas=ins["betas"], expression=ins["expression"], jaw_pose=ins["jaw"],
                    left_hand_pose=ins["lhand"], right_hand_pose=ins["rhand"])
        g = capi.ObjectiveGrads()
        for name, field in zip(OBJECTIVE_GRADS, capi.OBJECTIVE_GRADS):
            if like[name] is not None:
                grads[name] = torch.empty_like(like[name])
                setattr(g, "d_" + field + "_dev", grads[name].data_ptr())
    with torch.cuda.device(dev):
        capi.check(capi.load().sfx_objective_eval(C.byref(c), C.byref(a), C.byref(g) if g is not None else None, A.ptr(loss), A.stream(stream, dev)))
    return loss, grads


def camera_init_eval(joints, rotation, translation, focal_x, focal_y, center, gt_joints, init_count, joints_conf=None,
                     est_tz=None, data_weight=1.0, depth_loss_weight=0.0, use_conf=False, want_grads=True, stream=None):
    """SMPLifyCameraInitLoss.forward (fitting.py:499-520) and its gradient for B frames in one launch (sfx_camera_init_eval).
    Tensors as objective_eval; init_count [K]: how often keypoint k appears in init_joints_idxs; joints_conf [B, K] (use_conf:
    the broadcast of :509-511); est_tz [B] = trans_estimation[:, 2] or None (no depth term).
    Returns (loss [B], dict(joints=, rotation=, translation=))."""
    import torch
    B, K, joints = _obj_joints(joints)
    dev = joints.device
    arg = functools.partial(A.tensor, device=dev, optional=True, holder="joints")      # every other tensor: where joints is
    if use_conf and joints_conf is None:
        raise ValueError("use_conf needs joints_conf")
    ins = [joints, arg("rotation", rotation, (B, 3, 3)), arg("translation", translation, (B, 3)),
           arg("focal_x", focal_x, (B,)), arg("focal_y", focal_y, (B,)), arg("center", center, (B, 2)),
           arg("gt_joints", gt_joints, (B, K, 2)), arg("init_count", init_count, (K,)),
           arg("joints_conf", joints_conf, (B, K)) if use_conf else None, arg("est_tz", est_tz, (B,))]
    c = capi.CameraInitCfg()
    c.data_weight, c.depth_loss_weight, c.use_conf = float(data_weight), float(depth_loss_weight), int(bool(use_conf))
    loss = torch.empty([B], dtype=torch.float32, device=dev)
    grads = {}
    if want_grads:
        grads = dict(joints=torch.empty_like(ins[0]), rotation=torch.empty_like(ins[1]), translation=torch.empty_like(ins[2]))
    with torch.cuda.device(dev):
        capi.check(capi.load().sfx_camera_init_eval(C.byref(c), B, K, *[A.ptr(t) for t in ins], A.ptr(loss),
                                                    A.ptr(grads.get("joints")), A.ptr(grads.get("rotation")),
                                                    A.ptr(grads.get("translation")), A.stream(stream, dev)))
    return loss, grads


# ---- evaluation of fitted meshes (sfx_eval_align / sfx_eval_nearest, csrc/evaluate.hip) -------------------------------------
ALIGN_MODES = dict(none=0, procrustes=1, scale=2, pelvis=3)            # SFX_ALIGN_*
ALIGN_MAX_ANCHORS = 8                                                   # SFX_ALIGN_MAX_ANCHORS
NEAREST_MAX_THRESH = 8                                                  # SFX_NEAREST_MAX_THRESH


def _points(name, t):
    """(B, N) of a [B, N, 3] tensor; what it is and where it lives is left to A.tensor."""
    import torch
    if not torch.is_tensor(t):
        raise TypeError("%s: a torch tensor is needed, got %s" % (name, type(t).__name__))
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[1] < 1:
        raise ValueError("%s: shape %s, expected (B, N, 3) with N >= 1" % (name, tuple(t.shape)))
    return int(t.shape[0]), int(t.shape[1])


def _expect(name, t, *shapes, mask=False):
    """What a further argument is, refused before where ANY argument lives: a tensor of one of `shapes` and, for a mask, of
    torch.bool / torch.uint8; None passes.  A.tensor remains the single check of what is handed to the library, but it checks
    one tensor at a time, what it is before where it is, and every "what" of a call is to be refused before any "where"."""
    import torch
    if t is None:
        return
    if not torch.is_tensor(t):
        raise TypeError("%s: a torch tensor is needed, got %s" % (name, type(t).__name__))
    if tuple(t.shape) not in shapes:
        raise ValueError("%s: shape %s, expected %s" % (name, tuple(t.shape), " or ".join(str(tuple(n)) for n in shapes)))
    if mask and t.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s: torch.bool or torch.uint8 is needed, got %s" % (name, t.dtype))


def check_rho(rho):
    """rho of a robustified term as a float; refuses what the library would."""
    rho = float(rho)
    if not (np.isfinite(rho) and rho >= 0.0):
        raise ValueError("rho: %r, a finite value >= 0 is needed" % (rho,))
    return rho


_CACHE_SIZE = 8


def _cached(cache, key, make, size=_CACHE_SIZE):
    """cache[key] of an OrderedDict, made by make() on a miss (an insert beyond `size` drops the oldest entries, and with them
    whatever they held on a device); a hit marks the entry recent."""
    if key in cache:
        cache.move_to_end(key)
        return cache[key]
    ent = cache[key] = make()
    while len(cache) > size:
        cache.popitem(last=False)
    return ent


_scratch_cache = collections.OrderedDict()      # (term, device, sizes) -> the scratch tensors of that term's calls of that size


def _term_scratch(term, which, nbytes, dev, *sizes):
    """The scratch of a term's forward ('fwd') or backward ('bwd') for calls of one size on one device: made once and kept
    (the last few sizes), so calls of one size belong on one stream."""
    import torch
    ent = _cached(_scratch_cache, (term, dev) + sizes, dict)
    if which not in ent:
        ent[which] = torch.empty([max(1, nbytes // 4)], dtype=torch.int32, device=dev)
    return ent[which]


def _point_mask(name, mask, shape, dev, holder):
    import torch
    return A.tensor(name, mask, shape, device=dev, dtype=torch.uint8, optional=True, convert=True, holder=holder)


def align_errors(est, gt, mode="procrustes", mask=None, anchors=(2, 3), return_transform=False, stream=None):
    """Per-point error of B estimated point sets against their ground truth after an alignment (sfx_eval_align):
    mode 'none' (mpjpe / vertex_to_vertex_error, utils.py:597-614), 'procrustes' (ProcrustesAlignment, utils.py:540-595),
    'scale' (ScaleAlignment, utils.py:729-772) or 'pelvis' (PelvisAlignment, utils.py:650-668: each set moved by the mean of
    its own rows `anchors`).  est, gt: float32 contiguous CUDA tensors [B, N, 3]; mask: [B, N] torch.bool / torch.uint8 or
    None -- a masked point is left out of every sum and its error is exactly 0.
    Returns (err [B, N], mean [B]: the mean over the valid points), and xform [B, 13] (scale, R row-major, t of the map
    applied to the estimate; include/sfx.h) as a third value with return_transform.  Only enqueues on the current (or the
    given) stream."""
    import torch
    if mode not in ALIGN_MODES:
        raise ValueError("mode: one of %s, got %r" % (sorted(ALIGN_MODES), mode))
    B, N = _points("est", est)
    anc = None
    if mode == "pelvis":
        anc = capi.i32(list(anchors)).reshape(-1)
        if not 1 <= anc.size <= ALIGN_MAX_ANCHORS:
            raise ValueError("anchors: %d given, supported 1..%d" % (anc.size, ALIGN_MAX_ANCHORS))
        if anc.min() < 0 or anc.max() >= N:
            raise ValueError("anchors: %s outside the %d points" % (anc.tolist(), N))
    _expect("gt", gt, (B, N, 3))
    _expect("mask", mask, (B, N), mask=True)
    est = A.tensor("est", est, (B, N, 3))
    dev = est.device
    gt = A.tensor("gt", gt, (B, N, 3), device=dev, holder="est")
    mask = _point_mask("mask", mask, (B, N), dev, "est")
    err = torch.empty([B, N], dtype=torch.float32, device=dev)
    mean = torch.empty([B], dtype=torch.float32, device=dev)
    xform = torch.empty([B, 13], dtype=torch.float32, device=dev) if return_transform else None
    if B > 0:
        with torch.cuda.device(dev):
            capi.check(capi.load().sfx_eval_align(ALIGN_MODES[mode], B, N, A.ptr(est), A.ptr(gt), A.ptr(mask), capi.iptr(anc),
                                                  0 if anc is None else anc.size, A.ptr(err), A.ptr(mean), A.ptr(xform),
                                                  A.stream(stream, dev)))
    return (err, mean, xform) if return_transform else (err, mean)


def nearest_distances(a, b, thresholds=(), mask_a=None, mask_b=None, return_distances=True, stream=None):
    """The two nearest-neighbour queries of point_fscore (utils.py:622-648) for B pairs of point sets (sfx_eval_nearest):
    a [B, Na, 3], b [B, Nb, 3] float32 contiguous CUDA tensors, masks [B, Na] / [B, Nb] torch.bool / torch.uint8 or None;
    thresholds: up to 8 distances.  Returns a dict of tensors on the device:
      dist_ab [B, Na], dist_ba [B, Nb]     distance of every valid point to the nearest valid point of the other set, 0 at
                                           masked points (with return_distances)
      count_ab, count_ba [B, n_thresh]     int32: valid points nearer than each threshold
      valid [B, 2]                         int32: valid points of a and of b
    A set with no valid point gives distances 0 and counts 0.  Only enqueues on the current (or the given) stream."""
    import torch
    B, Na = _points("a", a)
    Nb = _points("b", b)[1]
    th = capi.f64(list(thresholds)).reshape(-1)
    if th.size > NEAREST_MAX_THRESH:
        raise ValueError("thresholds: %d given, at most %d" % (th.size, NEAREST_MAX_THRESH))
    _expect("b", b, (B, Nb, 3))
    _expect("mask_a", mask_a, (B, Na), mask=True)
    _expect("mask_b", mask_b, (B, Nb), mask=True)
    a = A.tensor("a", a, (B, Na, 3))
    dev = a.device
    b = A.tensor("b", b, (B, Nb, 3), device=dev, holder="a")
    mask_a = _point_mask("mask_a", mask_a, (B, Na), dev, "a")
    mask_b = _point_mask("mask_b", mask_b, (B, Nb), dev, "a")
    out = dict(count_ab=torch.empty([B, th.size], dtype=torch.int32, device=dev),           # (zeroed by the library)
               count_ba=torch.empty([B, th.size], dtype=torch.int32, device=dev),
               valid=torch.empty([B, 2], dtype=torch.int32, device=dev))
    if return_distances:
        out["dist_ab"] = torch.empty([B, Na], dtype=torch.float32, device=dev)
        out["dist_ba"] = torch.empty([B, Nb], dtype=torch.float32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            capi.check(capi.load().sfx_eval_nearest(B, Na, Nb, A.ptr(a), A.ptr(b), A.ptr(mask_a), A.ptr(mask_b), th.size,
                                                    capi.dptr(th), A.ptr(out.get("dist_ab")), A.ptr(out.get("dist_ba")),
                                                    A.ptr(out["count_ab"]), A.ptr(out["count_ba"]), A.ptr(out["valid"]),
                                                    A.stream(stream, dev)))
    return out


# ---- differentiable nearest-point term between point sets (sfx_chamfer_forward / _backward, csrc/chamfer.hip) ---------------
CHAMFER_MAX_POINTS = 1 << 26                                            # SFX_CHAMFER_MAX_POINTS


def chamfer_forward_scratch_bytes(B, Na, Nb):
    """SFX_CHAMFER_FORWARD_SCRATCH_BYTES of include/sfx.h."""
    return 4 * B * (Na + Nb)


def chamfer_backward_scratch_bytes(B, Na, Nb):
    """SFX_CHAMFER_BACKWARD_SCRATCH_BYTES of include/sfx.h."""
    return 4 * B * (4 * (Na + Nb) + 2)


def _chamfer_args(a, b, mask_a, mask_b, weight_a, weight_b, rho):
    """The checked inputs both chamfer calls share: sizes, tensors as the library reads them, rho."""
    B, Na = _points("a", a)
    Nb = _points("b", b)[1]
    rho = check_rho(rho)
    if Na > CHAMFER_MAX_POINTS or Nb > CHAMFER_MAX_POINTS:
        raise ValueError("a, b: %d and %d points, at most %d each" % (Na, Nb, CHAMFER_MAX_POINTS))
    _expect("b", b, (B, Nb, 3))
    _expect("mask_a", mask_a, (B, Na), mask=True)
    _expect("mask_b", mask_b, (B, Nb), mask=True)
    _expect("weight_a", weight_a, (B, Na))
    _expect("weight_b", weight_b, (B, Nb))
    a = A.tensor("a", a, (B, Na, 3))
    dev = a.device
    b = A.tensor("b", b, (B, Nb, 3), device=dev, holder="a")
    mask_a = _point_mask("mask_a", mask_a, (B, Na), dev, "a")
    mask_b = _point_mask("mask_b", mask_b, (B, Nb), dev, "a")
    weight_a = A.tensor("weight_a", weight_a, (B, Na), device=dev, optional=True, holder="a")
    weight_b = A.tensor("weight_b", weight_b, (B, Nb), device=dev, optional=True, holder="a")
    return B, Na, Nb, dev, a, b, mask_a, mask_b, weight_a, weight_b, rho


def chamfer_eval(a, b, mask_a=None, mask_b=None, weight_a=None, weight_b=None, rho=0.0, return_dist2=True, stream=None):
    """The nearest-point (chamfer) term of B pairs of point sets in both directions (sfx_chamfer_forward; the contract is in
    include/sfx.h): a [B, Na, 3], b [B, Nb, 3] float32 contiguous CUDA tensors; masks [B, Na] / [B, Nb] torch.bool / torch.uint8
    or None (a masked point is neither a query nor a target); weights [B, Na] / [B, Nb] float32 or None (a weight scales the
    point's own query term only); rho = 0: squared distances, rho > 0: the GMoF rho^2 s / (s + rho^2) of the squared distance.
    Returns a dict of device tensors:
      loss [B, 2]                          sum over a's points of w rho(s) to the nearest point of b, and the same for b against a
      idx_ab [B, Na], idx_ba [B, Nb]       int32: that nearest point (the lowest index of a tie), -1 at a masked point or where
                                           there is no target
      dist2_ab, dist2_ba                   its squared distance, float32 (with return_dist2)
      valid [B, 2]                         int32: valid points of a and of b
    Index and squared distance are numpy's float32 argmin / min bit for bit; a mesh's bits depend on its own points only.  Only
    enqueues on the current (or the given) stream; the scratch of a size is cached, so calls of one size belong on one stream."""
    import torch
    B, Na, Nb, dev, a, b, mask_a, mask_b, weight_a, weight_b, rho = _chamfer_args(a, b, mask_a, mask_b, weight_a, weight_b, rho)
    out = dict(loss=torch.empty([B, 2], dtype=torch.float32, device=dev),
               idx_ab=torch.empty([B, Na], dtype=torch.int32, device=dev), idx_ba=torch.empty([B, Nb], dtype=torch.int32, device=dev),
               valid=torch.empty([B, 2], dtype=torch.int32, device=dev))
    if return_dist2:
        out["dist2_ab"] = torch.empty([B, Na], dtype=torch.float32, device=dev)
        out["dist2_ba"] = torch.empty([B, Nb], dtype=torch.float32, device=dev)
    if B > 0:
        nbytes = chamfer_forward_scratch_bytes(B, Na, Nb)
        scratch = _term_scratch("chamfer", "fwd", nbytes, dev, B, Na, Nb)
        with torch.cuda.device(dev):
            capi.check(capi.load().sfx_chamfer_forward(
                B, Na, Nb, A.ptr(a), A.ptr(b), A.ptr(mask_a), A.ptr(mask_b), A.ptr(weight_a), A.ptr(weight_b), rho,
                A.ptr(out["idx_ab"]), A.ptr(out["idx_ba"]), A.ptr(out.get("dist2_ab")), A.ptr(out.get("dist2_ba")),
                A.ptr(out["loss"]), A.ptr(out["valid"]), A.ptr(scratch), nbytes, A.stream(stream, dev)))
    return out


def chamfer_backward(a, b, fwd, grad, want=("a", "b"), mask_a=None, mask_b=None, weight_a=None, weight_b=None, rho=0.0,
                     stream=None):
    """Gradient of the chamfer term with respect to the points (sfx_chamfer_backward): `fwd` is what chamfer_eval returned for
    the same inputs (its idx_ab and idx_ba are read), grad [B, 2] the upstream of loss; masks, weights and rho as in that call.
    want: which of 'a', 'b' to compute.  Returns (da [B, Na, 3] or None, db [B, Nb, 3] or None).  Every row is its own term plus
    the terms of the points that chose it, summed in float64 in ascending index through an inverted index built on the device:
    no float atomics, the same bits in every run and in any batch.  Only enqueues on the current (or the given) stream."""
    import torch
    want = tuple(want)
    if not want or [w for w in want if w not in ("a", "b")]:
        raise ValueError("want: some of ('a', 'b'), got %r" % (want,))
    B, Na, Nb, dev, a, b, mask_a, mask_b, weight_a, weight_b, rho = _chamfer_args(a, b, mask_a, mask_b, weight_a, weight_b, rho)
    if not isinstance(fwd, dict) or "idx_ab" not in fwd or "idx_ba" not in fwd:
        raise TypeError("fwd: the dict chamfer_eval returned is needed (idx_ab, idx_ba)")
    _expect("grad", grad, (B, 2))
    idx_ab = A.tensor("fwd['idx_ab']", fwd["idx_ab"], (B, Na), device=dev, dtype=torch.int32, holder="a")
    idx_ba = A.tensor("fwd['idx_ba']", fwd["idx_ba"], (B, Nb), device=dev, dtype=torch.int32, holder="a")
    grad = A.tensor("grad", grad, (B, 2), device=dev, holder="a")
    da = torch.empty([B, Na, 3], dtype=torch.float32, device=dev) if "a" in want else None
    db = torch.empty([B, Nb, 3], dtype=torch.float32, device=dev) if "b" in want else None
    if B > 0:
        nbytes = chamfer_backward_scratch_bytes(B, Na, Nb)
        scratch = _term_scratch("chamfer", "bwd", nbytes, dev, B, Na, Nb)
        with torch.cuda.device(dev):
            capi.check(capi.load().sfx_chamfer_backward(
                B, Na, Nb, A.ptr(a), A.ptr(b), A.ptr(mask_a), A.ptr(mask_b), A.ptr(weight_a), A.ptr(weight_b), rho,
                A.ptr(idx_ab), A.ptr(idx_ba), A.ptr(grad), A.ptr(da), A.ptr(db), A.ptr(scratch), nbytes, A.stream(stream, dev)))
    return da, db


# ---- a mesh topology as the device calls read it (point_mesh_*, render_meshes) --------------------------------------------------
_topology_cache = collections.OrderedDict()     # (faces object, V) -> the checked faces and what each device holds of them


def _checked_faces(faces, V):
    """`faces` as an int64 host array [F, 3] after the one check of its shape, dtype and vertex ids against V vertices."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
        raise ValueError("faces: an integer array of shape (F, 3) with F >= 1 is needed, got %s %s" % (f.dtype, f.shape))
    f = f.astype(np.int64)
    if V < 1 or f.min() < 0 or f.max() >= V:
        raise ValueError("faces: vertex ids %d..%d outside the %d vertices" % (f.min(), f.max(), V))
    return f


def _topology(faces, V):
    """The cache entry of a topology against V vertices: checked once per object, whatever lives where.  A tensor is recognised
    by its storage and version (the entry keeps it alive, so the address cannot be handed out again), anything else by its
    contents.  The entry holds the int32 host copy, F and, per device, what _topology_on keeps there."""
    import hashlib
    import torch
    if torch.is_tensor(faces):
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError("faces: shape %s, expected (F, 3) with F >= 1" % (tuple(faces.shape),))
        if faces.dtype not in (torch.int32, torch.int64):
            raise ValueError("faces: torch.int32 or torch.int64 is needed, got %s" % faces.dtype)
        key = ("tensor", faces.data_ptr(), faces._version, tuple(faces.shape), tuple(faces.stride()), faces.dtype, faces.device, V)
        host = faces.detach().cpu().numpy
    else:
        arr = np.ascontiguousarray(np.asarray(faces))
        key = ("host", hashlib.sha1(arr.tobytes()).hexdigest(), arr.shape, arr.dtype.str, V)
        host = lambda: arr

    def make():
        f = _checked_faces(host(), V)
        return dict(keep=faces, F=int(f.shape[0]), host=np.ascontiguousarray(f.astype(np.int32)), dev={})
    return _cached(_topology_cache, key, make)


def _topology_on(ent, dev):
    """What a topology entry holds on one device: `faces`, the int32 device copy, and whatever its callers keep beside it (it
    goes when the entry is evicted)."""
    import torch
    if dev not in ent["dev"]:
        ent["dev"][dev] = dict(faces=torch.as_tensor(ent["host"], device=dev))
    return ent["dev"][dev]


# ---- differentiable point-to-triangle term (sfx_p2m_forward / _backward, csrc/p2m.hip) -----------------------------------------
P2M_MAX_POINTS = 1 << 26                                                # SFX_P2M_MAX_POINTS


def p2m_forward_scratch_bytes(B, Np, Nv):
    """SFX_P2M_FORWARD_SCRATCH_BYTES of include/sfx.h."""
    return 4 * B * Np


def p2m_backward_scratch_bytes(B, Np, Nv):
    """SFX_P2M_BACKWARD_SCRATCH_BYTES of include/sfx.h."""
    return 4 * B * (9 * Np + 2 * Nv + 1)


def _p2m_args(points, vertices, faces, point_mask, point_weights, face_mask, rho):
    """The checked inputs both point-to-triangle calls share: sizes, tensors as the library reads them, rho."""
    B, Np = _points("points", points)
    Nv = _points("vertices", vertices)[1]
    rho = check_rho(rho)
    if Np > P2M_MAX_POINTS or Nv > P2M_MAX_POINTS:
        raise ValueError("points, vertices: %d and %d, at most %d each" % (Np, Nv, P2M_MAX_POINTS))
    _expect("vertices", vertices, (B, Nv, 3))
    topo = _topology(faces, Nv)
    F = topo["F"]
    if F > P2M_MAX_POINTS:
        raise ValueError("faces: %d faces, at most %d" % (F, P2M_MAX_POINTS))
    _expect("point_mask", point_mask, (B, Np), mask=True)
    _expect("face_mask", face_mask, (F,), (B, F), mask=True)
    if face_mask is not None and face_mask.dim() == 1:
        face_mask = face_mask[None].expand(B, F).contiguous()
    _expect("point_weights", point_weights, (B, Np))
    points = A.tensor("points", points, (B, Np, 3))
    dev = points.device
    vertices = A.tensor("vertices", vertices, (B, Nv, 3), device=dev, holder="points")
    point_mask = _point_mask("point_mask", point_mask, (B, Np), dev, "points")
    face_mask = _point_mask("face_mask", face_mask, (B, F), dev, "points")
    point_weights = A.tensor("point_weights", point_weights, (B, Np), device=dev, optional=True, holder="points")
    return B, Np, Nv, F, dev, points, vertices, _topology_on(topo, dev)["faces"], point_mask, point_weights, face_mask, rho


def point_mesh_eval(points, vertices, faces, point_mask=None, point_weights=None, face_mask=None, rho=0.0, return_dist2=True,
                    return_bary=True, stream=None):
    """The point-to-triangle term from B point clouds to the surfaces of B meshes of one topology (sfx_p2m_forward; the
    contract is in include/sfx.h): points [B, Np, 3], vertices [B, Nv, 3] float32 contiguous CUDA tensors; faces [F, 3] integers
    (a CUDA / CPU tensor or an array: checked once per object for shape, dtype and range, its device copy cached); point_mask
    [B, Np], face_mask [B, F] or [F] torch.bool / torch.uint8 or None (a masked point has no term, a masked face is no
    candidate); point_weights [B, Np] float32 or None; rho = 0: squared distances, rho > 0: the GMoF rho^2 s / (s + rho^2).
    Returns a dict of device tensors:
      loss [B]            sum over the valid points of w rho(s) to the nearest point of the mesh's triangles
      face [B, Np]        int32: the nearest face (the lowest index of a tie), -1 at a masked point or without a candidate
      bary [B, Np, 3]     (u, v, w) of the closest point on it (with return_bary)
      dist2 [B, Np]       its squared distance, float32 (with return_dist2)
      valid [B]           int32: valid points
    Face, squared distance and barycentrics are a float32 numpy restatement of the contract bit for bit; a mesh's bits depend
    on its own data only.  Only enqueues on the current (or the given) stream; the scratch of a size is cached, so calls of one
    size belong on one stream."""
    import torch
    B, Np, Nv, F, dev, points, vertices, faces, point_mask, point_weights, face_mask, rho = _p2m_args(
        points, vertices, faces, point_mask, point_weights, face_mask, rho)
    out = dict(loss=torch.empty([B], dtype=torch.float32, device=dev), face=torch.empty([B, Np], dtype=torch.int32, device=dev),
               valid=torch.empty([B], dtype=torch.int32, device=dev))
    if return_bary:
        out["bary"] = torch.empty([B, Np, 3], dtype=torch.float32, device=dev)
    if return_dist2:
        out["dist2"] = torch.empty([B, Np], dtype=torch.float32, device=dev)
    if B > 0:
        nbytes = p2m_forward_scratch_bytes(B, Np, Nv)
        scratch = _term_scratch("p2m", "fwd", nbytes, dev, B, Np, Nv)
        with torch.cuda.device(dev):
            capi.check(capi.load().sfx_p2m_forward(
                B, Np, Nv, F, A.ptr(points), A.ptr(vertices), A.ptr(faces), A.ptr(point_mask), A.ptr(face_mask),
                A.ptr(point_weights), rho, A.ptr(out["face"]), A.ptr(out.get("bary")), A.ptr(out.get("dist2")),
                A.ptr(out["loss"]), A.ptr(out["valid"]), A.ptr(scratch), nbytes, A.stream(stream, dev)))
    return out


def point_mesh_backward(points, vertices, faces, fwd, grad, want=("points", "vertices"), point_mask=None, point_weights=None,
                        rho=0.0, stream=None):
    """Gradient of the point-to-triangle term (sfx_p2m_backward): `fwd` is what point_mesh_eval returned for the same inputs
    (its face is read), grad [B] the upstream of loss; point_mask, point_weights and rho as in that call.  want: which of
    'points', 'vertices' to compute.  Returns (dp [B, Np, 3] or None, dv [B, Nv, 3] or None).  A point's row is c (p - q); a
    vertex's row sums -(c bary_k)(p - q) over the corners that name it, in float64 in ascending corner entry through an inverted
    index built on the device: no float atomics, the same bits in every run and in any batch.  Only enqueues on the current (or
    the given) stream."""
    import torch
    want = tuple(want)
    if not want or [w for w in want if w not in ("points", "vertices")]:
        raise ValueError("want: some of ('points', 'vertices'), got %r" % (want,))
    B, Np, Nv, F, dev, points, vertices, faces, point_mask, point_weights, _, rho = _p2m_args(
        points, vertices, faces, point_mask, point_weights, None, rho)
    if not isinstance(fwd, dict) or "face" not in fwd:
        raise TypeError("fwd: the dict point_mesh_eval returned is needed (face)")
    _expect("grad", grad, (B,))
    face = A.tensor("fwd['face']", fwd["face"], (B, Np), device=dev, dtype=torch.int32, holder="points")
    grad = A.tensor("grad", grad, (B,), device=dev, holder="points")
    dp = torch.empty([B, Np, 3], dtype=torch.float32, device=dev) if "points" in want else None
    dv = torch.empty([B, Nv, 3], dtype=torch.float32, device=dev) if "vertices" in want else None
    if B > 0:
        nbytes = p2m_backward_scratch_bytes(B, Np, Nv)
        scratch = _term_scratch("p2m", "bwd", nbytes, dev, B, Np, Nv)
        with torch.cuda.device(dev):
            capi.check(capi.load().sfx_p2m_backward(
                B, Np, Nv, F, A.ptr(points), A.ptr(vertices), A.ptr(faces), A.ptr(point_mask), A.ptr(point_weights), rho,
                A.ptr(face), A.ptr(grad), A.ptr(dp), A.ptr(dv), A.ptr(scratch), nbytes, A.stream(stream, dev)))
    return dp, dv


# ---- fitted meshes over their images (sfx_render_meshes, csrc/raster.hip) -----------------------------------------------------
RENDER_MAX_LIGHTS = capi.RENDER_MAX_LIGHTS
RENDER_BASE_RGB = (0.4, 0.4, 0.7)                                       # utils.py:499 vertex_colors
# The reference's scene in the fit camera's frame, as (direction towards the light, intensity): the three "raymond" lights of
# utils.py:467-495 (theta = pi / 6, phi = 0, 2 pi / 3, 4 pi / 3; they shine along -z of their own frame) and the light that
# scene.add(light) puts at the origin (utils.py:519-521), all of intensity 1.  The OpenGL camera looks down -z with y up; the
# fit camera looks down +z with y down, so y and z change sign.
RENDER_LIGHTS = tuple(((0.5 * np.cos(phi), -0.5 * np.sin(phi), -np.cos(np.pi / 6.0)), 1.0)
                      for phi in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0)) + (((0.0, 0.0, -1.0), 1.0),)
RENDER_MAX_PIXELS = 1 << 26     # pixels of one launch: the visibility buffer takes 8 bytes each (512 MB)
RENDER_WANT = ("rgba", "depth", "tri", "screen", "dropped")


def vertex_face_csr(faces, V):
    """The faces of every vertex of a triangle mesh, on the host: (offsets int32 [V + 1], face ids int32 [offsets[V]]) with the
    faces of vertex v at offsets[v] .. offsets[v + 1] - 1 in ascending face id, each face once (also one that names the vertex
    twice).  Deterministic: the order in which sfx_render_meshes sums a vertex's face normals."""
    V = int(V)
    f = _checked_faces(faces, V)
    F = f.shape[0]
    pairs = np.unique(f.reshape(-1) * F + np.repeat(np.arange(F, dtype=np.int64), 3))      # (vertex, face), sorted, each once
    offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(pairs // F, minlength=V), out=offsets[1:])
    return offsets.astype(np.int32), (pairs % F).astype(np.int32)


def _render_topology(faces, V, dev):
    """What render_meshes keeps of a topology on a device, beside the faces of _topology_on: the vertex -> face lists as device
    tensors and the scratch tensors of its calls."""
    import torch
    ent = _topology(faces, V)
    part = _topology_on(ent, dev)
    if "off" not in part:
        off, vf = vertex_face_csr(ent["host"], V)
        vf_pad = np.zeros(3 * ent["F"], np.int32)                      # (the C ABI's [3F])
        vf_pad[:vf.size] = vf
        part.update(F=ent["F"], scratch={}, off=torch.as_tensor(off, device=dev), vf=torch.as_tensor(vf_pad, device=dev))
    return part


def _render_scratch(ent, n, V, HW, dev):
    """vis int64 [n * HW], vnormal float32 [n, V, 3], snapped int32 [n, V, 2] of a topology's calls, grown on demand."""
    import torch
    sc = ent["scratch"]
    if sc.get("n_v", 0) < n:
        sc["vnormal"] = torch.empty([n, V, 3], dtype=torch.float32, device=dev)
        sc["snapped"] = torch.empty([n, V, 2], dtype=torch.int32, device=dev)
        sc["n_v"] = n
    if sc.get("n_px", 0) < n * HW:
        sc["vis"] = None                                               # (released before its replacement is asked for)
        sc["vis"] = torch.empty([n * HW], dtype=torch.int64, device=dev)
        sc["n_px"] = n * HW
    return sc


def render_cfg(base_rgb=RENDER_BASE_RGB, lights=RENDER_LIGHTS, znear=0.05):
    """sfx_render_cfg from a base colour, ((direction, intensity), ...) and the near plane; refuses what the library would."""
    lights = list(lights)
    if len(lights) > RENDER_MAX_LIGHTS:
        raise ValueError("lights: %d given, at most %d" % (len(lights), RENDER_MAX_LIGHTS))
    if not float(znear) > 0.0:
        raise ValueError("znear: %r, must be > 0" % (znear,))
    cfg = capi.RenderCfg()
    base = capi.f32(base_rgb).reshape(-1)
    if base.size != 3:
        raise ValueError("base_rgb: three values are needed, got %d" % base.size)
    cfg.base_rgb[:] = base.tolist()
    cfg.n_lights = len(lights)
    for l, (d, inten) in enumerate(lights):
        d = capi.f32(d).reshape(-1)
        if d.size != 3:
            raise ValueError("lights[%d]: a direction of three values is needed" % l)
        cfg.light_dir[l][:] = d.tolist()
        cfg.light_intensity[l] = float(inten)
    cfg.znear = float(znear)
    return cfg


def render_meshes(vertices, faces, translation, focal, center, H, W, rotation=None, background=None, want=("rgba",),
                  base_rgb=RENDER_BASE_RGB, lights=RENDER_LIGHTS, znear=0.05, max_pixels=RENDER_MAX_PIXELS, stream=None):
    """B meshes of one topology drawn through their fit cameras (sfx_render_meshes; the contract is in include/sfx.h): exact
    integer coverage with the top-left rule, perspective-correct depth, the nearest triangle per pixel (ties to the lowest id),
    smooth normals, Lambert shading by directional lights, composited over `background`.
      vertices [B, V, 3], translation [B, 3], center [B, 2]     float32 contiguous CUDA tensors
      focal          [B, 2] (fx, fy), [B], or a number
      faces          [F, 3] integers: a CUDA / CPU tensor or an array; its vertex -> face lists and device copies are cached per
                     (topology, device) together with the scratch buffers, so calls of one topology belong on one stream
      rotation       [B, 3, 3] or None (identity);  background uint8 [B, H, W, 3] or None (black)
      want           any of 'rgba' uint8 [B, H, W, 4] (alpha 255 on the mesh, 0 elsewhere), 'depth' float32 [B, H, W] (+inf where
                     empty), 'tri' int32 [B, H, W] (-1 where empty), 'screen' float32 [B, V, 3] (x, y, Z), 'dropped' int32 [B]
                     (triangles left out for a vertex behind znear, non-finite or beyond 2^20 pixels; there is no clipping)
      lights         ((direction towards the light in the camera frame, intensity), ...), at most 8
      max_pixels     the batch is walked in chunks of at most max_pixels // (H * W) meshes (at least one): the visibility buffer
                     takes 8 bytes per pixel.  An image does not depend on the chunking.
    Returns a dict of device tensors.  Only enqueues on the current (or the given) stream."""
    import torch
    want = tuple(want)
    bad = [w for w in want if w not in RENDER_WANT]
    if bad or not want:
        raise ValueError("want: some of %s, got %r" % (RENDER_WANT, want))
    cfg = render_cfg(base_rgb, lights, znear)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
        raise ValueError("H, W: %d x %d, both >= 1 and H * W within int32 are needed" % (H, W))
    B, V = _points("vertices", vertices)
    vertices = A.tensor("vertices", vertices, (B, V, 3))
    dev = vertices.device
    translation = A.tensor("translation", translation, (B, 3), device=dev, holder="vertices")
    center = A.tensor("center", center, (B, 2), device=dev, holder="vertices")
    if torch.is_tensor(focal):
        if focal.dim() == 1:
            focal = A.tensor("focal", focal, (B,), device=dev, holder="vertices").unsqueeze(1).expand(B, 2).contiguous()
        else:
            focal = A.tensor("focal", focal, (B, 2), device=dev, holder="vertices")
    else:
        focal = torch.full([B, 2], float(focal), dtype=torch.float32, device=dev)
    rotation = A.tensor("rotation", rotation, (B, 3, 3), device=dev, optional=True, holder="vertices")
    background = A.tensor("background", background, (B, H, W, 3), device=dev, dtype=torch.uint8, optional=True, holder="vertices")
    ent = _render_topology(faces, V, dev)
    out = {}
    if "rgba" in want:
        out["rgba"] = torch.empty([B, H, W, 4], dtype=torch.uint8, device=dev)
    if "depth" in want:
        out["depth"] = torch.empty([B, H, W], dtype=torch.float32, device=dev)
    if "tri" in want:
        out["tri"] = torch.empty([B, H, W], dtype=torch.int32, device=dev)
    if "screen" in want:
        out["screen"] = torch.empty([B, V, 3], dtype=torch.float32, device=dev)
    if "dropped" in want:
        out["dropped"] = torch.empty([B], dtype=torch.int32, device=dev)
    if B == 0:
        return out
    chunk = max(1, min(B, int(max_pixels) // (H * W), (2 ** 31 - 1) // (H * W)))
    sc = _render_scratch(ent, chunk, V, H * W, dev)
    lib = capi.load()

    def part(t, b0, b1):
        return None if t is None else A.ptr(t[b0:b1])
    with torch.cuda.device(dev):
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            capi.check(lib.sfx_render_meshes(
                C.byref(cfg), b1 - b0, V, ent["F"], H, W, part(vertices, b0, b1), A.ptr(ent["faces"]), A.ptr(ent["off"]),
                A.ptr(ent["vf"]), part(rotation, b0, b1), part(translation, b0, b1), part(focal, b0, b1), part(center, b0, b1),
                part(background, b0, b1), A.ptr(sc["vis"]), A.ptr(sc["vnormal"]), A.ptr(sc["snapped"]),
                part(out.get("rgba"), b0, b1), part(out.get("depth"), b0, b1), part(out.get("tri"), b0, b1),
                part(out.get("screen"), b0, b1), part(out.get("dropped"), b0, b1), A.stream(stream, dev)))
    return out


def prof_enable(on=True, every=1):
    """HIP-event timing of the named kernel launches; `every` = N times only every N-th launch of
    each name (an event pair costs two queue packets per launch)."""
    capi.load().sfx_prof_enable((int(on) & 3) | ((max(1, int(every)) & 0xffff) << 8))


def prof_reset():
    capi.load().sfx_prof_reset()


def prof_get(name):
    ms, n, u = C.c_double(), C.c_int64(), C.c_double()
    capi.load().sfx_prof_get(name.encode(), C.byref(ms), C.byref(n), C.byref(u))
    return ms.value, n.value, u.value


def loop_host_stats(reset=False):
    """Host side of the dense fitting loops since the last reset: seconds enqueueing, seconds waiting for stage flags, wall
    seconds, rounds (sfx_loop_host_stats)."""
    w = (C.c_double * 4)()
    capi.check(capi.load().sfx_loop_host_stats(w, int(bool(reset))))
    return dict(enqueue_s=w[0], wait_s=w[1], wall_s=w[2], rounds=int(w[3]))


def pen_work_reset():
    """Zero the device counters of the interpenetration term's work (sfx_pen_work_reset)."""
    capi.check(capi.load().sfx_pen_work_reset())


def pen_work_get():
    """Work of the interpenetration term since the last reset, counted on the device: grid entries and ordered pairs per
    column evaluation (a mesh that went through the broad phase), the number of those evaluations, surviving triangles."""
    w = (C.c_int64 * 6)()
    capi.check(capi.load().sfx_pen_work_get(w))
    cols = max(int(w[2]), 1)
    return dict(entries=int(w[0]), pairs=int(w[1]), columns=int(w[2]), survivors=int(w[3]),
                lists_overflowed=int(w[4]), walks_cut=int(w[5]),     # lists re-derived from the grid (exact); walks cut (> 0: pairs missing, order dependent)
                entries_per_column=w[0] / cols, pairs_per_column=w[1] / cols, survivors_per_column=w[3] / cols)


def pen_form(form=-1):
    """Debug / A-B: which form of the interpenetration term Penetration handles and FrameBatches created from now on take
    (sfx_debug_pen_form: 0 = the ten general kernels, the default; 1 = one workgroup per column behind the pair tests; 2 = form 1
    handing every column over).  LAB build only (include/sfx_lab.h).  Returns the previous setting; any other argument only queries."""
    capi.need_lab("pen_form")
    return int(capi.load().sfx_debug_pen_form(int(form)))


def pen_phase_ticks():
    """Debug: mean microseconds a column evaluation spent in the phases of k_pen_narrow since pen_work_reset()."""
    capi.need_lab("pen_phase_ticks")
    w = (C.c_int64 * 8)()
    capi.check(capi.load().sfx_debug_pen_phase_ticks(w))
    n = max(int(w[5]), 1)
    return dict(entry_us=w[0] / n / 100.0, list_us=w[1] / n / 100.0, eval_us=w[2] / n / 100.0, sums_us=w[3] / n / 100.0,
                verts_us=w[4] / n / 100.0, evaluations=int(w[5]), pairs_per_evaluation=w[6] / n)


def _warn_point2plane():
    import warnings
    warnings.warn("point2plane=True: the form built here -- Psi^2 (n_f . n_g)^2, gradient through both normals -- is assumption A6 of "
                  "oracle/penetration.py; the mesh_intersection package's own form is not available to compare with, so the numbers "
                  "may differ from the reference's (every shipped cfg leaves the flag False)", RuntimeWarning, stacklevel=3)


def _read_pairs(call):
    n = C.c_int32(0)
    capi.check(call(0, None, C.byref(n)))
    out = np.zeros((max(int(n.value), 1), 2), np.int32)
    capi.check(call(int(out.shape[0]), capi.iptr(out), C.byref(n)))
    return out[:int(n.value)].astype(np.int64)


class Penetration(capi.Handle):
    """Interpenetration term on a batch of posed meshes (sfx_pen_*):
    BVH + FilterFaces + DistanceFieldPenetrationLoss of the reference's external package
    (fitting.py:437-455).  `segm` / `parents`: per-face part labels (smplx_parts_segm.pkl);
    `ign_part_pairs`: the cfg's ["9,16", ...] strings or (a, b) tuples."""
    _destroy = "sfx_pen_destroy"

    def __init__(self, num_verts, faces, segm=None, parents=None, ign_part_pairs=None, max_collisions=128,
                 max_batch=1):
        self._lib = capi.load()
        faces = capi.i32(np.asarray(faces).astype(np.int64).reshape(-1, 3))
        self.V, self.F, self.max_batch = int(num_verts), int(faces.shape[0]), int(max_batch)
        ign = A.ign_pairs(ign_part_pairs)
        sg = capi.i32(segm) if segm is not None else None
        pr = capi.i32(parents) if parents is not None else None
        h = C.c_void_p()
        capi.check(self._lib.sfx_pen_create(self.V, self.F, capi.iptr(faces), capi.iptr(sg), capi.iptr(pr),
                                            capi.iptr(ign) if len(ign) else None, len(ign), int(max_collisions),
                                            self.max_batch, C.byref(h)))
        self._h = h

    def _verts(self, verts):
        return A.tensor("verts", verts, (None, self.V, 3), make_contiguous=True)

    def eval(self, verts, sigma, penalize_outside=True, stream=None, point2plane=False):
        """verts: float32 CUDA tensor [B, V, 3] -> (loss [B], d loss / d verts [B, V, 3]) on the GPU.
        point2plane: DistanceFieldPenetrationLoss(point2plane=True) (include/sfx.h sfx_pen_set_point2plane)."""
        if point2plane:
            _warn_point2plane()
        import torch
        v = self._verts(verts)
        capi.check(self._lib.sfx_pen_set_point2plane(self._h, int(bool(point2plane))))
        B = v.shape[0]
        loss = torch.empty([B], dtype=torch.float32, device=v.device)
        dv = torch.empty_like(v)
        capi.check(self._lib.sfx_pen_eval(self._h, B, A.ptr(v), float(sigma), int(bool(penalize_outside)), A.ptr(loss), A.ptr(dv),
                                          A.stream(stream)))
        return loss, dv

    def eval_pairs(self, verts, pairs, sigma, penalize_outside=True, point2plane=False, stream=None):
        """DistanceFieldPenetrationLoss on pairs the CALLER supplies (sfx_pen_eval_pairs): verts float32 CUDA [B, V, 3], pairs
        int32 CUDA [B, n, 2] (each unordered pair once; rows with -1 are empty) -> (loss [B], d loss / d verts [B, V, 3],
        d loss / d triangle corners [B, F, 3, 3])."""
        import torch
        if point2plane:
            _warn_point2plane()
        v = self._verts(verts)
        B = v.shape[0]
        pr = A.tensor("pairs", pairs, (B, None, 2), v.device, dtype=torch.int32, make_contiguous=True, holder="verts")
        capi.check(self._lib.sfx_pen_set_point2plane(self._h, int(bool(point2plane))))
        loss = torch.empty([B], dtype=torch.float32, device=v.device)
        dv = torch.empty_like(v)
        dtri = torch.empty([B, self.F, 3, 3], dtype=torch.float32, device=v.device)
        capi.check(self._lib.sfx_pen_eval_pairs(self._h, B, A.ptr(v), A.ptr(pr), int(pr.shape[1]), float(sigma),
                                                int(bool(penalize_outside)), A.ptr(loss), A.ptr(dv), A.ptr(dtri), A.stream(stream)))
        return loss, dv, dtri

    def stats(self, B):
        out = np.zeros((B, 4), np.int32)
        capi.check(self._lib.sfx_pen_stats(self._h, int(B), capi.iptr(out)))
        return dict(pairs=out[:, 0].copy(), dropped=out[:, 1].copy(), entry_overflow=out[:, 2].copy(), walks_cut=out[:, 3].copy())

    def pairs(self, mesh):
        """Ordered pair list [n, 2] (receiving triangle, partner; receiver ascending, partner ascending) of mesh `mesh` of the
        most recent eval(): both orders of every colliding pair, after the part filter and the max_collisions rule."""
        return _read_pairs(lambda cap, buf, n: self._lib.sfx_pen_pairs(self._h, int(mesh), cap, buf, n))

    def phase_clocks(self, B):
        """Debug (LAB build): the clock window of the first B meshes' stats rows, [B, 11] (sfx_pen_phase_clocks; PenClockCol in
        csrc/collide_slots.h).  Columns 3-6 (PEN_CLK_LIST, _EVAL, _SUMS, _VERTS): microseconds from k_pen_narrow's start to the
        ends of its phases D-G -- 0 in form 0 and for a mesh handed to the general kernels.  Column 9 (PEN_CLK_WALKS_CUT) and
        column 10 (PEN_CLK_ENTRIES) are counts, returned as they are.  Columns 0-2 and 7-8 have no writer: 0."""
        capi.need_lab("phase_clocks")
        out = np.zeros((B, 11), np.int32)
        capi.check(self._lib.sfx_pen_phase_clocks(self._h, int(B), capi.iptr(out)))
        res = out / 100.0
        res[:, 9:] = out[:, 9:]
        return res
