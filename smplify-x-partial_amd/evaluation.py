"""Accuracy metrics either side of the fitting path: the alignment / error
utilities of smplifyx/utils.py:540-801 and `compute_v2v` of smplifyx/eval.py:13-45, used to score
fitted meshes against ground truth (EHF).  Same class and function names and return structures as the
reference.  Two paths:
  host    numpy, the default: what the classes below compute when called.  The F-score uses a k-d tree
          (scipy) for the nearest-neighbour distances the reference obtains from open3d.
  device  `compute_v2v(..., device=True)` and `point_fscore` on GPU tensors: the alignments, the errors
          and the nearest-neighbour queries run in HIP (engine.align_errors / engine.nearest_distances,
          csrc/evaluate.hip) on meshes that already sit in device memory, and the results stay there.
          No scipy, no copy to the host.
Nothing here runs inside the optimisation.
"""
from collections import defaultdict

import numpy as np


def _as_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def mpjpe(input_joints, target_joints):
    """Per-joint Euclidean error, [..., J] (utils.py:597-611)."""
    d = np.asarray(input_joints) - np.asarray(target_joints)
    return np.sqrt((d * d).sum(axis=-1))


def vertex_to_vertex_error(input_vertices, target_vertices):
    return mpjpe(input_vertices, target_vertices)


def point_fscore(pred, gt, thresh):
    """Precision / recall / F of two point sets at a distance threshold (utils.py:622-648).  GPU tensors ([N, 3] and
    [M, 3]) are scored on the device (engine.nearest_distances) and give 0-d float64 device tensors; anything else
    takes the host path."""
    if getattr(pred, "is_cuda", False) and getattr(gt, "is_cuda", False):
        from . import engine
        nn = engine.nearest_distances(pred.unsqueeze(0), gt.unsqueeze(0), [thresh], return_distances=False)
        f, precision, recall = _fscore_from_counts(nn)
        return {"fscore": f[0, 0], "precision": precision[0, 0], "recall": recall[0, 0]}
    from scipy.spatial import cKDTree
    pred, gt = _as_np(pred), _as_np(gt)
    gt_to_pred = cKDTree(pred).query(gt)[0]
    pred_to_gt = cKDTree(gt).query(pred)[0]
    recall = (pred_to_gt < thresh).sum() / len(pred_to_gt)
    precision = (gt_to_pred < thresh).sum() / len(gt_to_pred)
    f = 2 * recall * precision / (recall + precision) if recall + precision > 0.0 else 0.0
    return {"fscore": f, "precision": precision, "recall": recall}


def _fscore_from_counts(nn):
    """(F, precision, recall), float64 [B, n_thresh] on the device, from the integer counts of engine.nearest_distances
    (a = the prediction); 0 / 0 (an empty set) takes the reference's F = 0 branch (utils.py:639-642)."""
    import torch
    valid = nn["valid"].double()
    recall = nn["count_ab"].double() / valid[:, 0:1]
    precision = nn["count_ba"].double() / valid[:, 1:2]
    f = torch.where(recall + precision > 0.0, 2 * recall * precision / (recall + precision), torch.zeros_like(recall))
    return f, precision, recall


def _cols(S1, S2):
    """Points as columns [d, N]; remembers whether the inputs were [N, d]."""
    S1, S2 = np.asarray(S1), np.asarray(S2)
    flip = S1.shape[0] not in (2, 3)
    if flip:
        S1, S2 = S1.T, S2.T
    assert S2.shape[1] == S1.shape[1]
    return S1, S2, flip


class ProcrustesAlignment(object):
    """Similarity transform (scale, rotation, translation) of S1 closest to S2 in the least-squares
    sense (orthogonal Procrustes / Umeyama; utils.py:540-595); returns the transformed S1."""

    def __repr__(self):
        return "ProcrustesAlignment"

    def __call__(self, S1, S2):
        S1, S2, flip = _cols(S1, S2)
        mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
        X1, X2 = S1 - mu1, S2 - mu2
        var1 = np.sum(X1 ** 2)
        K = X1 @ X2.T
        U, _, Vh = np.linalg.svd(K)
        Z = np.eye(U.shape[0])
        Z[-1, -1] *= np.sign(np.linalg.det(U @ Vh))          # det(R) = +1
        R = Vh.T @ Z @ U.T
        scale = np.trace(R @ K) / var1
        out = scale * (R @ S1) + (mu2 - scale * (R @ mu1))
        return out.T if flip else out


class ScaleAlignment(object):
    """Isotropic scale + translation only (utils.py:729-772)."""

    def __repr__(self):
        return "ScaleAlignment"

    def __call__(self, S1, S2):
        S1, S2, flip = _cols(S1, S2)
        mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
        scale = np.sqrt(np.sum((S2 - mu2) ** 2) / np.sum((S1 - mu1) ** 2))
        out = scale * S1 + (mu2 - scale * mu1)
        return out.T if flip else out


class PelvisAlignment(object):
    """Subtract the mean of the hip joints (utils.py:650-668)."""

    def __init__(self, hips_idxs=None):
        self.hips_idxs = [2, 3] if hips_idxs is None else hips_idxs

    def align_by_pelvis(self, joints):
        pelvis = joints[self.hips_idxs, :].mean(axis=0, keepdims=True)
        return {"joints": joints - pelvis, "pelvis": pelvis}

    def __call__(self, gt, est):
        return self.align_by_pelvis(gt)["joints"], self.align_by_pelvis(est)["joints"]


class PelvisAlignmentMPJPE(PelvisAlignment):
    def __init__(self, fscore_thresholds=None):
        super(PelvisAlignmentMPJPE, self).__init__()
        self.fscore_thresholds = fscore_thresholds

    def __call__(self, est_points, gt_points):
        gt_al, est_al = super(PelvisAlignmentMPJPE, self).__call__(gt_points, est_points)
        fscore = {t: point_fscore(est_al, gt_points, t) for t in (self.fscore_thresholds or [])}
        return {"point": mpjpe(est_al, gt_al), "fscore": fscore}


class ProcrustesAlignmentMPJPE(ProcrustesAlignment):
    def __init__(self, fscore_thresholds=None):
        super(ProcrustesAlignmentMPJPE, self).__init__()
        self.fscore_thresholds = fscore_thresholds

    def __call__(self, est_points, gt_points):
        aligned = super(ProcrustesAlignmentMPJPE, self).__call__(est_points, gt_points)
        fscore = {t: point_fscore(aligned, gt_points, t) for t in (self.fscore_thresholds or [])}
        return {"point": vertex_to_vertex_error(aligned, gt_points), "fscore": fscore}


# what the device path scores: exactly these classes (a subclass may override __call__) -> engine.align_errors mode
_DEVICE_MODES = {ProcrustesAlignmentMPJPE: "procrustes", PelvisAlignmentMPJPE: "pelvis"}


def _compute_v2v_device(fitted, target, alignments, vids, masks):
    import torch
    from . import engine
    for name, align in alignments.items():
        if type(align) not in _DEVICE_MODES:
            raise TypeError("alignments[%r]: the device path scores ProcrustesAlignmentMPJPE and PelvisAlignmentMPJPE "
                            "objects only, got %s" % (name, type(align).__name__))
    for what, t in (("vertices_fitted", fitted), ("vertices_target", target)):
        if not torch.is_tensor(t):
            raise TypeError("%s: a torch tensor is needed with device=True, got %s" % (what, type(t).__name__))
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("%s: shape %s, expected (B, N, 3)" % (what, tuple(t.shape)))
    if fitted.shape != target.shape:
        raise ValueError("vertices_target: shape %s, vertices_fitted %s" % (tuple(target.shape), tuple(fitted.shape)))
    for what, t in (("vertices_fitted", fitted), ("vertices_target", target)):
        if t.device.type != "cuda":
            raise ValueError("%s: a CUDA tensor is needed (no CPU fallback), got device %s" % (what, t.device))
    if vids is not None:
        idx = torch.as_tensor(np.asarray(vids), dtype=torch.long, device=fitted.device)
        fitted, target = fitted.index_select(1, idx), target.index_select(1, idx)
    fitted, target = fitted.float().contiguous(), target.float().contiguous()
    err, fs = {}, {}
    for name, align in alignments.items():
        mode = _DEVICE_MODES[type(align)]
        e, _, xf = engine.align_errors(fitted, target, mode=mode, mask=masks, anchors=getattr(align, "hips_idxs", (2, 3)),
                                       return_transform=True)
        err[name] = e
        fs[name] = {}
        thresholds = list(align.fscore_thresholds or [])
        if thresholds:
            # the aligned estimate against the ground truth AS GIVEN: for the pelvis alignment that is the reference's
            # quirk (utils.py:691-693).  xform in float64, the points rounded to float32 once
            x = xf.double()
            Rt = x[:, 1:10].reshape(-1, 3, 3).transpose(1, 2)
            p = fitted.double()
            aligned = (x[:, 0, None, None] * (p[..., 0:1] * Rt[:, None, 0] + p[..., 1:2] * Rt[:, None, 1] + p[..., 2:3] * Rt[:, None, 2])
                       + x[:, None, 10:13]).float()
            for i in range(0, len(thresholds), engine.NEAREST_MAX_THRESH):
                part = thresholds[i:i + engine.NEAREST_MAX_THRESH]
                nn = engine.nearest_distances(aligned, target, part, mask_a=masks, mask_b=masks, return_distances=False)
                f = _fscore_from_counts(nn)[0]
                for k, t in enumerate(part):
                    fs[name][t] = f[:, k]
    return {"point": err, "fscore": fs}


def compute_v2v(vertices_fitted, vertices_target, alignments, vids=None, masks=None, device=False):
    """Per-vertex errors of a batch under each alignment (eval.py:13-45):
    {'point': {name: [B, V]}, 'fscore': {name: {thresh: [B]}}}.
    device=True: both inputs are GPU tensors [B, N, 3], every alignment is exactly a ProcrustesAlignmentMPJPE or a
    PelvisAlignmentMPJPE of this module, and the same structure comes back holding torch tensors ON THE DEVICE (float32
    errors, float64 F-scores formed from integer counts): nothing synchronises until the caller reads.  vids selects points
    on the device; masks ([B, N] bool, applied after vids; the reference scores another in-bounds vertex subset per frame,
    eval.py:102-121) takes points out of a mesh's alignment, errors and F-score.  'point' holds 0 at masked-out points, so
    a mesh's mean error is  point.sum(1) / masks.sum(1)  -- the sum divided by the valid count, not point.mean(1)."""
    if device:
        return _compute_v2v_device(vertices_fitted, vertices_target, alignments, vids, masks)
    if masks is not None:
        raise ValueError("masks: per-mesh masks are a feature of the device path (device=True)")
    fitted, target = _as_np(vertices_fitted), _as_np(vertices_target)
    if vids is not None:
        fitted, target = fitted[:, vids], target[:, vids]
    err, fs = {}, {}
    for name, align in alignments.items():
        rows, f = [], defaultdict(list)
        for b in range(target.shape[0]):
            out = align(fitted[b], target[b])
            rows.append(out["point"])
            for t, v in out["fscore"].items():
                f[t].append(np.asarray(v["fscore"]).copy())
        err[name] = np.stack(rows)
        fs[name] = {t: np.stack(v) for t, v in f.items()}
    return {"point": err, "fscore": fs}


def read_ply_vertices(path):
    """xyz of the first element of a binary-little-endian or ascii .ply (the vertices.ply written
    by fit_single_frame, fit_single_frame.py:671-677)."""
    with open(path, "rb") as fh:
        fmt, n, props = None, 0, 0
        first = True
        while True:
            line = fh.readline().decode("ascii").strip()
            if line.startswith("format"):
                fmt = line.split()[1]
            elif line.startswith("element") and first:
                n = int(line.split()[2]); first = False
            elif line.startswith("element"):
                first = None
            elif line.startswith("property") and first is False:
                props += 1
            elif line == "end_header":
                break
        if fmt == "binary_little_endian":
            return np.frombuffer(fh.read(n * props * 4), "<f4").reshape(n, props)[:, :3].copy()
        if fmt == "ascii":
            return np.array([[float(v) for v in fh.readline().split()[:3]] for _ in range(n)], np.float32)
        raise ValueError("unsupported ply format %r" % fmt)
