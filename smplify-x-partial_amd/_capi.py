"""ctypes binding of include/sfx.h (libsfx.so).  Thin: argument marshalling only.

The library is the product path; there is no Python/CPU fallback.  `load()` raises if the
shared object is missing (run `python __graft_entry__.py` or csrc/build.sh) and
`sfx_model_create` fails loudly when no HIP device is present.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFX_LIB", os.path.join(_HERE, "libsfx.so"))
_lib = None

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
f64p = C.POINTER(C.c_double)


class ModelDesc(C.Structure):
    _fields_ = [
        ("V", C.c_int32), ("F", C.c_int32), ("J", C.c_int32),
        ("num_betas", C.c_int32), ("num_expr", C.c_int32), ("num_pca", C.c_int32),
        ("v_template", f32p), ("shapedirs", f32p), ("posedirs", f32p), ("J_regressor", f32p),
        ("lbs_weights", f32p), ("parents", i32p), ("hands_comp_l", f32p), ("hands_comp_r", f32p),
        ("pose_mean", f32p), ("faces", i32p),
        ("n_extra", C.c_int32), ("extra_vertex_ids", i32p),
        ("n_lmk", C.c_int32), ("lmk_faces_idx", i32p), ("lmk_bary", f32p),
        ("n_dyn_rows", C.c_int32), ("n_dyn", C.c_int32), ("dyn_lmk_faces_idx", i32p), ("dyn_lmk_bary", f32p),
        ("K", C.c_int32), ("joint_map", i32p),
    ]


class StageWeights(C.Structure):
    _fields_ = [
        ("body_pose_weight", C.c_float), ("shape_weight", C.c_float),
        ("hand_prior_weight", C.c_float), ("expr_prior_weight", C.c_float),
        ("jaw_prior_weight", C.c_float * 3),
        ("hand_joint_weight", C.c_float), ("face_joint_weight", C.c_float),
        ("coll_loss_weight", C.c_float), ("bending_prior_weight", C.c_float),
    ]


class StageWeights64(C.Structure):
    """sfx_stage_weights_f64: the stage weights of a float64 batch (high_precision = 2)."""
    _fields_ = [
        ("body_pose_weight", C.c_double), ("shape_weight", C.c_double),
        ("hand_prior_weight", C.c_double), ("expr_prior_weight", C.c_double),
        ("jaw_prior_weight", C.c_double * 3),
        ("hand_joint_weight", C.c_double), ("face_joint_weight", C.c_double),
        ("coll_loss_weight", C.c_double), ("bending_prior_weight", C.c_double),
    ]


class BatchCfg(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("n_stages", C.c_int32), ("use_vposer", C.c_int32),
        ("use_hands", C.c_int32), ("use_face", C.c_int32), ("use_joints_conf", C.c_int32),
        ("has_regression_pose", C.c_int32), ("use_conf_cam_init", C.c_int32),
        ("num_body_joints", C.c_int32), ("maxiters", C.c_int32),
        ("ftol", C.c_double), ("gtol", C.c_double),
        ("lr", C.c_float), ("rho", C.c_float), ("depth_loss_weight", C.c_float),
        ("lbs_mode", C.c_int32), ("reuse_entry_eval", C.c_int32),
        ("side_view_thsh", C.c_float), ("left_shoulder_idx", C.c_int32), ("right_shoulder_idx", C.c_int32),
        ("interpenetration", C.c_int32), ("max_collisions", C.c_int32), ("df_cone_height", C.c_float),
        ("penalize_outside", C.c_int32), ("slots", C.c_int32),
        ("lbfgs_tolerance_grad", C.c_double), ("lbfgs_tolerance_change", C.c_double),
        ("lbfgs_max_eval", C.c_int32), ("lbfgs_history_size", C.c_int32), ("lbfgs_max_iter", C.c_int32), ("high_precision", C.c_int32),
        ("point2plane", C.c_int32),
    ]


class OptCfg(C.Structure):
    """sfx_opt_cfg: B problems of N variables, run_fitting's tolerances and the hyper-parameters of lbfgs_ls.LBFGS."""
    _fields_ = [
        ("B", C.c_int32), ("N", C.c_int32), ("n_groups", C.c_int32), ("group_len", C.c_int32 * 12),
        ("maxiters", C.c_int32), ("ftol", C.c_double), ("gtol", C.c_double), ("lr", C.c_float),
        ("tolerance_grad", C.c_double), ("tolerance_change", C.c_double),
        ("max_iter", C.c_int32), ("max_eval", C.c_int32), ("history_size", C.c_int32), ("reuse_entry_eval", C.c_int32),
    ]


class OptWideCfg(C.Structure):
    """sfx_opt_wide_cfg: as OptCfg, with the group lengths behind a HOST pointer (up to 256 of them)."""
    _fields_ = [
        ("B", C.c_int32), ("N", C.c_int32), ("n_groups", C.c_int32), ("group_len", C.POINTER(C.c_int32)),
        ("maxiters", C.c_int32), ("ftol", C.c_double), ("gtol", C.c_double), ("lr", C.c_float),
        ("tolerance_grad", C.c_double), ("tolerance_change", C.c_double),
        ("max_iter", C.c_int32), ("max_eval", C.c_int32), ("history_size", C.c_int32), ("reuse_entry_eval", C.c_int32),
    ]


class ObjectiveCfg(C.Structure):
    """sfx_objective_cfg: weights, flags and pose-prior form of SMPLifyLoss for sfx_objective_eval (pointers: DEVICE)."""
    _fields_ = [
        ("rho", C.c_float), ("data_weight", C.c_float), ("body_pose_weight", C.c_float), ("shape_weight", C.c_float),
        ("bending_prior_weight", C.c_float), ("hand_prior_weight", C.c_float), ("expr_prior_weight", C.c_float),
        ("jaw_prior_weight", C.c_float * 3),
        ("use_joints_conf", C.c_int32), ("use_hands", C.c_int32), ("use_face", C.c_int32), ("prior_form", C.c_int32),
        ("gmm_M", C.c_int32), ("gmm_D", C.c_int32),
        ("gmm_means_dev", C.c_void_p), ("gmm_precisions_dev", C.c_void_p), ("gmm_nll_weights_dev", C.c_void_p),
        ("gmm_comp_const_dev", C.c_void_p),
    ]


# the tensors of sfx_objective_in / sfx_objective_grads, in the structures' order
OBJECTIVE_INPUTS = ("joints", "cam_rot", "cam_t", "focal_x", "focal_y", "center", "gt_joints", "joints_conf", "joint_weights",
                    "body_pose", "prior", "prior_target", "betas", "expression", "jaw", "lhand", "rhand")
OBJECTIVE_GRADS = ("joints", "cam_rot", "cam_t", "body_pose", "prior", "betas", "expression", "jaw", "lhand", "rhand")


class ObjectiveIn(C.Structure):
    _fields_ = ([("B", C.c_int32), ("K", C.c_int32), ("n_prior", C.c_int32), ("num_betas", C.c_int32), ("num_expr", C.c_int32)]
                + [(n + "_dev", C.c_void_p) for n in OBJECTIVE_INPUTS])


class ObjectiveGrads(C.Structure):
    _fields_ = [("d_" + n + "_dev", C.c_void_p) for n in OBJECTIVE_GRADS]


class CameraInitCfg(C.Structure):
    _fields_ = [("data_weight", C.c_float), ("depth_loss_weight", C.c_float), ("use_conf", C.c_int32)]


RENDER_MAX_LIGHTS = 8       # SFX_RENDER_MAX_LIGHTS


class RenderCfg(C.Structure):
    """sfx_render_cfg: base colour, directional lights (camera frame, towards the light) and the near plane of sfx_render_meshes."""
    _fields_ = [("base_rgb", C.c_float * 3), ("n_lights", C.c_int32), ("light_dir", (C.c_float * 3) * RENDER_MAX_LIGHTS),
                ("light_intensity", C.c_float * RENDER_MAX_LIGHTS), ("znear", C.c_float)]


# every symbol include/sfx.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sfx_model_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]),
    "sfx_model_destroy": (None, [C.c_void_p]),
    "sfx_model_set_parts": (C.c_int, [C.c_void_p, i32p, i32p, i32p, C.c_int32]),
    "sfx_model_set_vposer": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [f32p] * 6),
    "sfx_vposer_create": (C.c_int, [C.c_int32, C.c_int32] + [f32p] * 6 + [C.POINTER(C.c_void_p)]),
    "sfx_vposer_destroy": (None, [C.c_void_p]),
    "sfx_vposer_decode": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_vposer_decode_backward": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # latent, hidden, n_in, bn1 (w, b, mean, var), fc1 (w, b), bn2 (w, b, mean, var), fc2 (w, b), mu (w, b), logvar (w, b), out
    "sfx_vposer_encoder_create": (C.c_int, [C.c_int32] * 3 + [f32p] * 16 + [C.POINTER(C.c_void_p)]),
    "sfx_vposer_encoder_destroy": (None, [C.c_void_p]),
    "sfx_vposer_encode": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_vposer_encode_backward": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_void_p]),
    "sfx_lbs_forward": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 12 + [C.c_void_p]),
    # model, B, nine inputs, dvertices, djoints, nine gradients, stream
    "sfx_lbs_backward": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 20 + [C.c_void_p]),
    "sfx_batch_create": (C.c_int, [C.c_void_p, C.POINTER(BatchCfg), C.POINTER(StageWeights), C.POINTER(C.c_void_p)]),
    "sfx_batch_destroy": (None, [C.c_void_p]),
    "sfx_batch_set_frames": (C.c_int, [C.c_void_p] + [f32p] * 5),
    "sfx_batch_set_params": (C.c_int, [C.c_void_p] + [f32p] * 11),
    "sfx_batch_get_params": (C.c_int, [C.c_void_p] + [f32p] * 11),
    "sfx_batch_num_vars": (C.c_int, [C.c_void_p, C.c_int32]),
    "sfx_batch_closure": (C.c_int, [C.c_void_p, C.c_int32, f32p, f32p, C.c_void_p]),
    "sfx_batch_guess_init": (C.c_int, [C.c_void_p, i32p, C.c_int32, C.c_void_p]),
    "sfx_batch_fit": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sfx_batch_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, f32p, C.c_void_p]),
    "sfx_batch_pen_stats": (C.c_int, [C.c_void_p, i32p, i32p]),
    "sfx_batch_get_grad": (C.c_int, [C.c_void_p, C.c_int32, f32p]),
    "sfx_batch_set_stage_weights_f64": (C.c_int, [C.c_void_p, C.POINTER(StageWeights64)]),
    "sfx_batch_set_frames_f64": (C.c_int, [C.c_void_p] + [f64p] * 5),
    "sfx_batch_set_params_f64": (C.c_int, [C.c_void_p] + [f64p] * 11),
    "sfx_batch_get_params_f64": (C.c_int, [C.c_void_p] + [f64p] * 11),
    "sfx_batch_closure_f64": (C.c_int, [C.c_void_p, C.c_int32, f64p, f64p, C.c_void_p]),
    "sfx_batch_get_grad_f64": (C.c_int, [C.c_void_p, C.c_int32, f64p]),
    "sfx_batch_get_stats": (C.c_int, [C.c_void_p, f32p, i32p, i32p]),
    "sfx_lbfgs_two_loop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "sfx_batch_trace": (C.c_int, [C.c_void_p, C.c_int32]),
    "sfx_batch_get_trace": (C.c_int, [C.c_void_p, f32p, i32p]),
    "sfx_batch_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_opt_create": (C.c_int, [C.POINTER(OptCfg), C.POINTER(C.c_void_p)]),
    "sfx_opt_destroy": (None, [C.c_void_p]),
    # handle, mode, resume, x0, x_trial, stream
    "sfx_opt_begin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # handle, loss, grad, x_trial, stream
    "sfx_opt_tell": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_opt_active": (C.c_int, [C.c_void_p, i32p, C.c_void_p]),
    "sfx_opt_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, f32p, i32p, i32p]),
    "sfx_opt_trace": (C.c_int, [C.c_void_p, C.c_int32]),
    "sfx_opt_get_trace": (C.c_int, [C.c_void_p, f32p, i32p]),
    # the same eight for problems of up to 32768 variables (csrc/opt_wide.hip): the same signatures but for the configuration
    "sfx_opt_wide_create": (C.c_int, [C.POINTER(OptWideCfg), C.POINTER(C.c_void_p)]),
    "sfx_opt_wide_destroy": (None, [C.c_void_p]),
    "sfx_opt_wide_begin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_opt_wide_tell": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_opt_wide_active": (C.c_int, [C.c_void_p, i32p, C.c_void_p]),
    "sfx_opt_wide_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, f32p, i32p, i32p]),
    "sfx_opt_wide_trace": (C.c_int, [C.c_void_p, C.c_int32]),
    "sfx_opt_wide_get_trace": (C.c_int, [C.c_void_p, f32p, i32p]),
    # cfg, in, grads (or NULL), loss, stream
    "sfx_objective_eval": (C.c_int, [C.POINTER(ObjectiveCfg), C.POINTER(ObjectiveIn), C.POINTER(ObjectiveGrads), C.c_void_p, C.c_void_p]),
    # cfg, B, K, joints, rotation, translation, focal x / y, center, gt, init_count, conf, est_tz, loss, three gradients, stream
    "sfx_camera_init_eval": (C.c_int, [C.POINTER(CameraInitCfg), C.c_int32, C.c_int32] + [C.c_void_p] * 14 + [C.c_void_p]),
    # mode, B, N, est, gt, mask, anchors (host), n_anchors, err, mean, xform, stream
    "sfx_eval_align": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 3 + [i32p, C.c_int32] + [C.c_void_p] * 3 + [C.c_void_p]),
    # B, Na, Nb, a, b, mask_a, mask_b, n_thresh, thresh (host), dist_ab, dist_ba, count_ab, count_ba, valid, stream
    "sfx_eval_nearest": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 4 + [C.c_int32, f64p] + [C.c_void_p] * 5 + [C.c_void_p]),
    # B, Na, Nb, a, b, mask_a, mask_b, weight_a, weight_b, rho, idx_ab, idx_ba, dist2_ab, dist2_ba, loss, valid, scratch,
    # scratch_bytes, stream
    "sfx_chamfer_forward": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p]),
    # B, Na, Nb, a, b, mask_a, mask_b, weight_a, weight_b, rho, idx_ab, idx_ba, grad, da, db, scratch, scratch_bytes, stream
    "sfx_chamfer_backward": (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]),
    # B, Np, Nv, F, p, v, faces, mask_p, mask_f, weight_p, rho, face, bary, dist2, loss, valid, scratch, scratch_bytes, stream
    "sfx_p2m_forward": (C.c_int, [C.c_int32] * 4 + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]),
    # B, Np, Nv, F, p, v, faces, mask_p, weight_p, rho, face, grad, dp, dv, scratch, scratch_bytes, stream
    "sfx_p2m_backward": (C.c_int, [C.c_int32] * 4 + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
    # cfg, B, V, F, H, W, verts, faces, vf_offsets, vf_faces, rot, t, focal, center, background, three scratch buffers,
    # rgba, depth, tri, screen, dropped, stream
    "sfx_render_meshes": (C.c_int, [C.POINTER(RenderCfg)] + [C.c_int32] * 5 + [C.c_void_p] * 17 + [C.c_void_p]),
    "sfx_pen_create": (C.c_int, [C.c_int32, C.c_int32, i32p, i32p, i32p, i32p, C.c_int32, C.c_int32, C.c_int32,
                                 C.POINTER(C.c_void_p)]),
    "sfx_pen_destroy": (None, [C.c_void_p]),
    "sfx_pen_eval": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_pen_set_point2plane": (C.c_int, [C.c_void_p, C.c_int32]),
    "sfx_pen_eval_pairs": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfx_pen_stats": (C.c_int, [C.c_void_p, C.c_int32, i32p]),
    "sfx_pen_pairs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, i32p, C.POINTER(C.c_int32)]),
    "sfx_batch_pen_pairs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, i32p, C.POINTER(C.c_int32)]),
    "sfx_batch_pen_flags": (C.c_int, [C.c_void_p, i32p]),
    "sfx_batch_pen_launches": (C.c_int, [C.c_void_p]),
    "sfx_pen_work_reset": (C.c_int, []),
    "sfx_pen_work_get": (C.c_int, [C.POINTER(C.c_int64)]),
    "sfx_batch_set_gmm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, f32p, f32p, f32p]),
    "sfx_batch_set_gmm_form": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, f32p, f32p, f32p, f32p]),
    "sfx_batch_debug_read": (C.c_int, [C.c_void_p, C.c_char_p, f32p, C.c_int64]),
    "sfx_loop_host_stats": (C.c_int, [C.POINTER(C.c_double), C.c_int32]),
    "sfx_prof_enable": (C.c_int, [C.c_int32]),
    "sfx_prof_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "sfx_prof_reset": (None, []),
    "sfx_last_error": (C.c_char_p, []),
    "sfx_version": (C.c_char_p, []),
}

# what include/sfx_lab.h adds (libsfx_lab.so: csrc/build.sh with SFX_LAB=1; selected with SFX_LIB=<path> in the environment)
LAB_SYMBOLS = {
    "sfx_debug_lbs_dense_form": (C.c_int, [C.c_int32]),
    "sfx_debug_phase_clocks": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "sfx_pen_phase_clocks": (C.c_int, [C.c_void_p, C.c_int32, i32p]),
    "sfx_debug_pen_form": (C.c_int, [C.c_int32]),
    "sfx_debug_pen_phase_ticks": (C.c_int, [C.POINTER(C.c_int64)]),
    "sfx_debug_clocks": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
}
_has_lab = False


def has_lab():
    """True when the loaded library is the lab build (A/B forms, phase clocks: include/sfx_lab.h)."""
    load()
    return _has_lab


def need_lab(what):
    if not has_lab():
        raise RuntimeError("%s needs the lab build of the library (include/sfx_lab.h): SFX_LAB=1 bash "
                           "smplify-x-partial_amd/csrc/build.sh, then SFX_LIB=smplify-x-partial_amd/libsfx_lab.so" % what)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libsfx.so not built (%s): run `python __graft_entry__.py` "
                           "or smplify-x-partial_amd/csrc/build.sh; there is no CPU fallback" % LIB_PATH)
    # torch ships its own copy of the HIP runtime: it must be the one this process initialises, so
    # that libsfx.so (linked against libamdhip64 by soname) shares it with the torch tensors whose
    # data_ptr()s it is handed.  Loading libsfx first makes two runtimes meet in one process and
    # the second sees no device.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    global _has_lab
    _has_lab = all(hasattr(lib, name) for name in LAB_SYMBOLS)
    if _has_lab:
        for name, (res, args) in LAB_SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


class SfxError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise SfxError("libsfx error %d: %s" % (rc, load().sfx_last_error().decode()))


class Handle(object):
    """Owner of one library handle: `_lib`, `_h` and their release.  A subclass names its destroy symbol in `_destroy` and
    sets `_lib` / `_h` once its create call has succeeded; before that (an __init__ that raised) close() finds nothing to do."""
    _destroy = None
    _lib = None
    _h = None

    def close(self):
        h, self._h = self._h, None
        if h:
            getattr(self._lib, self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:       # (interpreter shutdown: the library or this module may be half gone)
            pass


def fptr(a):
    """numpy float32 C-contiguous array -> float* (None -> NULL).  Keeps no reference."""
    if a is None:
        return None
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(f32p)


def iptr(a):
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(i32p)


def f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def dptr(a):
    """numpy float64 C-contiguous array -> double* (None -> NULL).  Keeps no reference."""
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(f64p)


def f64(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)
