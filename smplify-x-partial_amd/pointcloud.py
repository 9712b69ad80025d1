"""3D data term: the nearest-point (chamfer) distance between mesh vertices and a point cloud, differentiable, on the device
(sfx_chamfer_forward / sfx_chamfer_backward, csrc/chamfer.hip; the contract is in include/sfx.h).

    loss = ChamferLoss(rho=0.05)(vertices, points)        # [B, 2]: mesh -> points, points -> mesh
    (loss[:, 0] + loss[:, 1]).sum().backward()

The caller weights and sums the two columns; loss[:, 1] alone is the one-sided term for a partial cloud (every observed point
near the mesh, no penalty for mesh regions nobody saw).  Both directions are point-to-point: points -> mesh is the distance to
the nearest mesh VERTEX, not to the nearest triangle, so the vertex spacing of the mesh bounds its accuracy.

PointToMeshLoss is the point-to-SURFACE term of the points -> mesh direction (sfx_p2m_forward / sfx_p2m_backward, csrc/p2m.hip):
every cloud point against the nearest point of the mesh's triangles.  A two-sided scan term adds it to ChamferLoss column 0:

    surface = PointToMeshLoss(faces, rho=0.05)(vertices, points)               # [B]
    loss = surface + ChamferLoss(rho=0.05)(vertices, points)[:, 0]"""
import torch
import torch.nn as nn

from . import engine

REDUCTIONS = ("mean", "sum")


def _first_derivatives_only():
    """Called by a backward: autograd records the backward pass only under create_graph=True."""
    if torch.is_grad_enabled():
        raise RuntimeError("backward(create_graph=True): the differentiable loss has first derivatives only -- its gradient "
                           "is computed by the device kernel, there is no graph of it to differentiate")


class _PointSetLoss(nn.Module):
    """What the point-set terms share: rho and the reduction, the inputs as the device reads them, the mean over the valid."""

    def __init__(self, rho=0.0, reduction="mean"):
        super().__init__()
        rho = engine.check_rho(rho)
        if reduction not in REDUCTIONS:
            raise ValueError("reduction: one of %s, got %r" % (REDUCTIONS, reduction))
        self.rho, self.reduction = rho, reduction

    @staticmethod
    def _float32(vertices, points, *weights):
        """vertices and points as float32 (differentiable casts), then the weights as float32 constants (None stays None)."""
        for name, t in (("vertices", vertices), ("points", points)):
            if not torch.is_tensor(t):
                raise TypeError("%s: a torch tensor is needed, got %s" % (name, type(t).__name__))
            if not t.is_floating_point():
                raise ValueError("%s: a floating-point tensor is needed, got %s" % (name, t.dtype))
        return [vertices.to(torch.float32).contiguous(), points.to(torch.float32).contiguous()] + [
            w.detach().to(torch.float32).contiguous() if torch.is_tensor(w) else w for w in weights]

    def _reduced(self, loss, valid, dtype):
        if self.reduction == "mean":
            loss = loss / valid.clamp(min=1).to(loss.dtype)
        return loss.to(dtype)


class _Chamfer(torch.autograd.Function):
    """loss [B, 2] of engine.chamfer_eval; backward: engine.chamfer_backward at the indices the forward found, for the inputs
    that need a gradient.  First derivatives only: backward(create_graph=True) is refused."""

    @staticmethod
    def forward(ctx, a, b, mask_a, mask_b, weight_a, weight_b, rho):
        fwd = engine.chamfer_eval(a.detach(), b.detach(), mask_a, mask_b, weight_a, weight_b, rho, return_dist2=False)
        ctx.save_for_backward(a.detach(), b.detach(), fwd["idx_ab"], fwd["idx_ba"])
        ctx.consts = (mask_a, mask_b, weight_a, weight_b, rho)
        ctx.mark_non_differentiable(fwd["valid"])
        return fwd["loss"], fwd["valid"]

    @staticmethod
    def backward(ctx, dloss, _dvalid):
        _first_derivatives_only()
        a, b, idx_ab, idx_ba = ctx.saved_tensors
        mask_a, mask_b, weight_a, weight_b, rho = ctx.consts
        want = tuple(n for n, need in zip(("a", "b"), ctx.needs_input_grad[:2]) if need)
        da = db = None
        if want:
            da, db = engine.chamfer_backward(a, b, dict(idx_ab=idx_ab, idx_ba=idx_ba), dloss.to(torch.float32).contiguous(), want,
                                             mask_a, mask_b, weight_a, weight_b, rho)
        return da, db, None, None, None, None, None


class ChamferLoss(_PointSetLoss):
    """forward(vertices [B, Nv, 3], points [B, Np, 3], vertex_mask=None, point_mask=None, vertex_weights=None,
    point_weights=None) -> [B, 2]: column 0 is mesh -> points (every valid vertex to its nearest valid point), column 1 is
    points -> mesh.  Per point the term is w rho(s) of the squared distance s: rho = 0 gives s itself, rho > 0 the GMoF
    rho^2 s / (s + rho^2) (smplifyx/utils.py:92-95).  A masked point ([B, N] torch.bool / torch.uint8, False = out) is neither a
    query nor a target; a weight ([B, N]) scales the point's own term only and receives no gradient.
    reduction 'mean' divides each column by its number of valid query points (at least 1), 'sum' returns the sums.
    Differentiable with respect to `vertices` and `points` (first derivatives only).  The arithmetic is float32 on the device
    whatever the inputs are: float64 tensors are converted for the call, and the loss and the gradients come back in the
    dtype of `vertices`.  Tensors must be on the GPU: there is no CPU fallback."""

    def forward(self, vertices, points, vertex_mask=None, point_mask=None, vertex_weights=None, point_weights=None):
        a, b, wa, wb = self._float32(vertices, points, vertex_weights, point_weights)
        loss, valid = _Chamfer.apply(a, b, vertex_mask, point_mask, wa, wb, self.rho)
        return self._reduced(loss, valid, vertices.dtype)


class _PointToMesh(torch.autograd.Function):
    """loss [B] of engine.point_mesh_eval; backward: engine.point_mesh_backward at the faces the forward found, for the inputs
    that need a gradient.  First derivatives only: backward(create_graph=True) is refused."""

    @staticmethod
    def forward(ctx, vertices, points, faces, point_mask, point_weights, face_mask, rho):
        fwd = engine.point_mesh_eval(points.detach(), vertices.detach(), faces, point_mask, point_weights, face_mask, rho,
                                     return_dist2=False, return_bary=False)
        ctx.save_for_backward(vertices.detach(), points.detach(), fwd["face"])
        ctx.consts = (faces, point_mask, point_weights, rho)
        ctx.mark_non_differentiable(fwd["valid"])
        return fwd["loss"], fwd["valid"]

    @staticmethod
    def backward(ctx, dloss, _dvalid):
        _first_derivatives_only()
        vertices, points, face = ctx.saved_tensors
        faces, point_mask, point_weights, rho = ctx.consts
        want = tuple(n for n, need in zip(("vertices", "points"), ctx.needs_input_grad[:2]) if need)
        dp = dv = None
        if want:
            dp, dv = engine.point_mesh_backward(points, vertices, faces, dict(face=face), dloss.to(torch.float32).contiguous(), want,
                                                point_mask, point_weights, rho)
        return dv, dp, None, None, None, None, None


class PointToMeshLoss(_PointSetLoss):
    """PointToMeshLoss(faces, rho=0.0, reduction='mean'); forward(vertices [B, Nv, 3], points [B, Np, 3], point_mask=None,
    point_weights=None, face_mask=None) -> [B]: every valid cloud point against the nearest point of the mesh's triangles
    (`faces` [F, 3] integers, one topology for the batch).  Per point the term is w rho(s) of the squared distance s to the
    surface: rho = 0 gives s itself, rho > 0 the GMoF rho^2 s / (s + rho^2).  A masked point ([B, Np] torch.bool / torch.uint8,
    False = out) has no term; a masked face ([B, F] or [F]) is no candidate; a weight ([B, Np]) scales the point's term and
    receives no gradient.  reduction 'mean' divides by the number of valid points (at least 1), 'sum' returns the sums.
    Differentiable with respect to `vertices` and `points` (first derivatives only): the closest point's barycentrics minimise,
    so the gradient flows through the point and the three corners of its face alone.  The arithmetic is float32 on the device
    whatever the inputs are: float64 tensors are converted for the call, and the loss and the gradients come back in the
    dtype of `vertices`.  Tensors must be on the GPU: there is no CPU fallback."""

    def __init__(self, faces, rho=0.0, reduction="mean"):
        super().__init__(rho, reduction)
        self.faces = faces

    def forward(self, vertices, points, point_mask=None, point_weights=None, face_mask=None):
        v, p, w = self._float32(vertices, points, point_weights)
        loss, valid = _PointToMesh.apply(v, p, self.faces, point_mask, w, face_mask, self.rho)
        return self._reduced(loss, valid, vertices.dtype)
