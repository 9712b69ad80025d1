"""Host-side helpers of the fitting path -- mirror of the reference's `utils` names that
the hot path touches (smplifyx/utils.py:60-95 rel_change/JointMapper/GMoF, :98-250
smpl_to_annotation, :306-436 _compute_euler_from_matrix, :438-538 optimization_visualization / render_mesh).  Index tables are
data; the euler conversion is a closed form, not the reference's generic scipy-style routine; the overlay is drawn by the
engine's rasteriser (csrc/raster.hip), not by pyrender.
"""
import numpy as np
import torch
import torch.nn as nn


def rel_change(prev_val, curr_val):
    """(prev - cur) / max(|prev|, |cur|, 1)  -- signed, utils.py:60-61."""
    return (prev_val - curr_val) / max([np.abs(prev_val), np.abs(curr_val), 1])


class JointMapper(nn.Module):
    """index_select(joints, 1, joint_maps); identity when no map (utils.py:68-81)."""

    def __init__(self, joint_maps=None):
        super().__init__()
        if joint_maps is None:
            self.joint_maps = None
        else:
            self.register_buffer("joint_maps", torch.as_tensor(np.asarray(joint_maps), dtype=torch.long))

    def forward(self, joints, **kwargs):
        if self.joint_maps is None:
            return joints
        return torch.index_select(joints, 1, self.joint_maps)


class GMoF(nn.Module):
    """rho^2 r^2 / (r^2 + rho^2), element-wise (utils.py:84-95).  Stand-alone module of the
    call surface; inside the fitting loop the robustifier lives in the HIP loss kernel."""

    def __init__(self, rho=1):
        super().__init__()
        self.rho = rho

    def extra_repr(self):
        return "rho = {}".format(self.rho)

    def forward(self, residual):
        sq = residual ** 2
        return self.rho ** 2 * torch.div(sq, sq + self.rho ** 2)


# ---- keypoint -> model-joint index tables (data) -------------------------------------------
# SMPL-X joint numbering: 0..54 kinematic joints, 55..75 vertex joints, 76..126 static face
# landmarks, 127..143 dynamic contour.
_SMPLX_BODY = {
    "coco25": [55, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7,
               56, 57, 58, 59, 60, 61, 62, 63, 64, 65],
    "halpe": [55, 57, 56, 59, 58, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8,
              15, 12, 0, 60, 63, 61, 64, 62, 65],
    "coco_wholebody": [55, 57, 56, 59, 58, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8,
                       60, 61, 62, 63, 64, 65],
    "coco19": [55, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 56, 57, 58, 59],
}
# wrist, then (index, middle, pinky->ring order of OpenPose) 3 joints + tip each
_FINGER_ORDER = [(37, 66), (25, 67), (28, 68), (34, 69), (31, 70)]   # thumb,index,middle,ring,pinky


def _hand(wrist, first, tip0):
    out = [wrist]
    for base, tip in _FINGER_ORDER:
        b = base + first
        out += [b, b + 1, b + 2, tip + tip0]
    return out


def smpl_to_annotation(model_type="smplx", use_hands=True, use_face=True,
                       use_face_contour=False, format="coco25"):
    """Indices that reorder SMPL-X joints into the keypoint format (utils.py:98-250).
    Only model_type 'smplx' is on the supported path."""
    if model_type != "smplx":
        raise ValueError("Unknown model type: {}".format(model_type))
    fmt = format if format == "coco19" else format.lower()
    if fmt not in _SMPLX_BODY:
        raise ValueError("Unknown joint format: {}".format(format))
    parts = [np.array(_SMPLX_BODY[fmt], dtype=np.int32)]
    shift = -6 if fmt == "coco19" else 0          # coco19 has no foot keypoints: 6 fewer vertex joints
    if use_hands:
        parts.append(np.array(_hand(20, 0, shift), dtype=np.int32))
        parts.append(np.array(_hand(21, 15, shift + 5), dtype=np.int32))
    if use_face:
        start = 76 + shift
        parts.append(np.arange(start, start + 51 + 17 * use_face_contour, dtype=np.int32))
    return np.concatenate(parts)


def euler_xyz_from_matrix(R):
    """Intrinsic x-y-z Euler angles of rotation matrices [...,3,3] -> [...,3].

    The reference converts regressor rotation matrices with a port of scipy's
    `as_euler('xyz')` for intrinsic rotations (utils.py:306-436) and then feeds the triples
    to the optimiser AS IF they were axis-angle vectors (fit_single_frame.py:212-235) -- a
    quirk this engine reproduces.  For R = Rx(a) Ry(b) Rz(c):
        b = asin(R02), a = atan2(-R12, R22), c = atan2(-R01, R00)
    which equals the reference's output away from gimbal lock (|b| = pi/2; there the
    reference sets c = 0 and a = atan2(R10 -/+ R01, R00 +/- R11))."""
    R = np.asarray(R, np.float64)
    r02 = np.clip(R[..., 0, 2], -1.0, 1.0)
    b = np.arcsin(r02)
    a = np.arctan2(-R[..., 1, 2], R[..., 2, 2])
    c = np.arctan2(-R[..., 0, 1], R[..., 0, 0])
    lock = np.abs(np.abs(b) - np.pi / 2) < 1e-7
    if np.any(lock):
        pos = r02 > 0
        # gimbal lock: third angle 0, first angle = the remaining in-plane rotation
        a_l = np.where(pos, np.arctan2(R[..., 1, 0], R[..., 1, 1]),
                       np.arctan2(-R[..., 1, 0], R[..., 1, 1]))
        a = np.where(lock, a_l, a)
        c = np.where(lock, 0.0, c)
    return np.stack([a, b, c], axis=-1)


def regression_prior_pose(regression_prior, expose=None, pixie=None, pare=None):
    """Initial body pose [63] and global orientation [3] from regressor outputs
    (fit_single_frame.py:209-235): every 3x3 rotation -> xyz-euler triple; 'combined' takes
    ExPose joints 0..18 and PIXIE joints 19..20, global orientation from ExPose."""
    if regression_prior in ("PIXIE", "combined"):
        pixie_pose = euler_xyz_from_matrix(np.asarray(pixie["body_pose"]))
        glob = euler_xyz_from_matrix(np.asarray(pixie["global_pose"]))[0]
    if regression_prior in ("ExPose", "combined"):
        expose_pose = euler_xyz_from_matrix(np.asarray(expose["body_pose"]))
        glob = euler_xyz_from_matrix(np.asarray(expose["global_orient"]))[0]
    if regression_prior == "PARE":
        pp = np.asarray(pare["pred_pose"])
        pare_pose = euler_xyz_from_matrix(pp[0, 1:22])
        glob = euler_xyz_from_matrix(pp[0, :1])[0]
    if regression_prior == "PIXIE":
        pose = pixie_pose
    elif regression_prior == "ExPose":
        pose = expose_pose
    elif regression_prior == "PARE":
        pose = pare_pose
    elif regression_prior == "combined":
        pose = np.concatenate([expose_pose[:19], pixie_pose[19:]])
    else:
        raise ValueError("Unknown regression prior: {}".format(regression_prior))
    return pose.reshape(-1).astype(np.float32), glob.astype(np.float32)


# ---- the fitted mesh over its image (utils.py:438-538) -------------------------------------------------------------------------
def _image_u8(img):
    """An image as uint8 [H, W, 3]: uint8 as it is, a float image in 0..1 rounded (floor(255 c + 0.5), so an image that came
    from uint8 / 255 gets its own bytes back; the reference truncates, which can lose a level)."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return np.ascontiguousarray(img[..., :3])
    return np.floor(np.clip(img[..., :3].astype(np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def render_mesh(img, mesh_trimesh, camera_center, camera_transl, focal_length, img_width, img_height):
    """render_mesh of the reference (utils.py:497-538) with its signature and conventions, drawn by engine.render_meshes:
    `mesh_trimesh` is any object with .vertices [V, 3] and .faces [F, 3] ALREADY rotated by 180 degrees about x, `camera_transl`
    has its x NEGATED (both as optimization_visualization hands them over, utils.py:454-460), `img` is a float image in 0..1
    (or uint8).  The two conventions place an OpenGL camera that looks down -z; together they are the fit camera's projection
    with R = I, so both are undone here and the engine is asked.  Returns uint8 [H, W, 3]: the mesh colour where the mesh
    covers a pixel, the image elsewhere (utils.py:531-536).  The shading is the engine's Lambert model under the reference's
    lights, not pyrender's metallic-roughness shader."""
    from . import engine
    dev = torch.device("cuda", torch.cuda.current_device())
    verts = np.asarray(mesh_trimesh.vertices, np.float32) * np.array([1.0, -1.0, -1.0], np.float32)
    transl = np.asarray(camera_transl, np.float32).reshape(3) * np.array([-1.0, 1.0, 1.0], np.float32)
    H, W = int(img_height), int(img_width)
    bg = _image_u8(img)
    if bg.shape != (H, W, 3):
        raise ValueError("img: shape %s, expected (%d, %d, 3)" % (bg.shape, H, W))
    out = engine.render_meshes(torch.as_tensor(verts[None], device=dev), np.asarray(mesh_trimesh.faces),
                               torch.as_tensor(transl[None], device=dev), float(focal_length),
                               torch.as_tensor(np.asarray(camera_center, np.float32).reshape(1, 2), device=dev), H, W,
                               background=torch.as_tensor(bg[None], device=dev))
    return out["rgba"][0, :, :, :3].cpu().numpy()


class _Mesh(object):
    """The two attributes render_mesh reads (trimesh is not a dependency of this engine)."""

    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


def optimization_visualization(img, smplx_path, pose_embedding, body_model, camera, focal_length, W, H, out_img_save_path,
                               vposer_rendered_img_save_path, use_cuda, mesh_fn, **kwargs):
    """optimization_visualization of the reference (utils.py:438-465): the body model's current mesh over `img`, written to
    `out_img_save_path` with PIL.  As there, the model is evaluated with body_pose = `pose_embedding`, the mesh is rotated by 180
    degrees about x and the camera's translation gets its x negated before render_mesh sees them.  Not drawn: the VPoser pose
    thumbnail (`vposer_rendered_img_save_path`: human_body_prior's renderer); not written: `mesh_fn` (trimesh's exporter)."""
    if not out_img_save_path:
        return
    from PIL import Image
    with torch.no_grad():
        vertices = body_model(return_verts=True, body_pose=pose_embedding).vertices.detach().cpu().numpy().squeeze()
        mesh = _Mesh(vertices * np.array([1.0, -1.0, -1.0]), body_model.faces)       # rotation by pi about x
        camera_center = camera.center.detach().cpu().numpy().squeeze().copy()
        camera_transl = camera.translation.detach().cpu().numpy().squeeze().copy()
        camera_transl[0] *= -1.0
        Image.fromarray(render_mesh(img, mesh, camera_center, camera_transl, focal_length, W, H)).save(out_img_save_path)
