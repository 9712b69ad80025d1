"""Closure gradient parity per parameter block (helpers.check_closure_blocks) on the MI355X.

helpers.check_closure bounds the gradient error over the whole variable vector, and one block carries almost all of that
vector's norm (the jaw prior at the far points of closure_probe, the pose near the solution): the hand PCA back-projection, the
expression columns of the shape basis, the eye joints, the gather through the per-stage variable table and the per-block column
ranges of the dense gradient GEMM could be wrong by orders of magnitude more than the bound says.  Here every block of every
stage is held to max(CLOSURE_GRAD_TOL, 10 x the float32 oracle's own error in that block against the float64 oracle).

  (a) far points       the suite's own closure tests call the block check at their call sites (closure_probe: body / full x rows /
                       dense; VPoser; halpe; use_pca off; the float64 batch); this file adds nothing to them but (c)
  (b) near points      test_gpu_parity.near_points: seeded, from the frames' ground truth, no fit: residual about one pixel
  (c) rows vs dense    the dense gradient against the rows gradient per block, at both point sets, under the same bound

B = 2 or 3 frames: batch sizes and tile edges are test_gpu_edges' (bit for bit)."""
import numpy as np
import pytest

import helpers as H
import test_gpu_parity as T
from test_gpu_parity import gpu      # noqa: F401  (the GPU fixture of the parity tests)

pytestmark = pytest.mark.gpu


def _cfg(which):
    if which == "body":
        return H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    if which == "full":
        return H.load_cfg("fit_smplx_combined_coco25.yaml")
    if which == "halpe":       # (as test_gpu_edges.test_halpe_closure_matches_oracle: K = 26, 3 stages, without the interpenetration term)
        return H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=False)
    assert which == "vposer"
    return H.load_cfg("fit_smplx_smplifyx.yaml")


def point_set(model, which, pts):
    """(cfg, frames, P with est_tz, oracle cache key) of point set `pts` ('far': closure_probe's / the VPoser test's own points;
    'near') of cfg `which`."""
    cfg = _cfg(which)
    vp = bool(cfg.get("use_vposer"))
    B, seed = (2, 5) if vp else (3, 11)
    if pts == "near":
        B, seed = 2, 23
    frames = T.synth_frames(model, cfg, 3 if vp else B)
    frames = {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in frames.items()}
    nemb = cfg.get("vposer_latent_dim", 32) if vp else None
    P, est = T.far_points(frames, B, seed, nemb=nemb) if pts == "far" else T.near_points(frames, B, nemb=nemb, seed=seed)
    P["est_tz"] = est
    return cfg, frames, P, (T._cfg_key(cfg), pts, B, seed)


_DEVICE = {}


def device_closures(model, which, pts, mode):
    """{stage: (loss [B], grad [B, N])} of the HIP closure at the point set, camera stage and every body stage."""
    if (which, pts, mode) in _DEVICE:
        return _DEVICE[which, pts, mode]
    from smplifyx_amd import synthetic
    cfg, frames, P, _ = point_set(model, which, pts)
    vp = bool(cfg.get("use_vposer"))
    dm = T._dm(model, cfg, **({"vposer": synthetic.make_synthetic_vposer(0)} if vp else {}))
    B = P["est_tz"].shape[0]
    fb = H.engine_batch_from_frames(dm, cfg, frames, range(B), lbs_mode=mode)
    fb.set_frames(frames["keypoints"], T._jw(cfg, frames), T._cmask(cfg, frames), frames["focal"],
                  np.tile([frames["W"] * 0.5, frames["H"] * 0.5], (B, 1)), 1000.0 / frames["H"], est_tz=P["est_tz"])
    Q = {k: v for k, v in P.items() if k != "est_tz"}
    if vp:
        fb.set_params(**Q)
    else:
        fb.set_params(regression_pose=frames["reg_pose"], **Q)
    out = {}
    for stage in [-1] + list(range(fb.n_stages)):
        loss, grad = fb.closure(stage)
        assert grad.shape == (B, fb.num_vars(stage))
        out[stage] = (loss, grad)
    fb.close(); dm.close()
    _DEVICE[which, pts, mode] = out
    return out


def oracle_closures(model, which, pts, stage):
    """(loss [B], go [B, N], go32 [B, N], blocks) of the oracle at the point set (one CPU evaluation per session)."""
    cfg, frames, P, key = point_set(model, which, pts)
    rows = [T._oracle_closure_blocks(model, cfg, frames, i, P, stage, key=key) for i in range(P["est_tz"].shape[0])]
    return np.array([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), rows[0][3]


@pytest.mark.parametrize("mode", ["rows", "dense"])
@pytest.mark.parametrize("which", ["body", "full", "halpe", "vposer"])
def test_near_solution_closure_matches_oracle_per_block(gpu, synth_model, which, mode):
    """Set (b).  The float32 oracle's own whole-vector error reaches 7e-6 (body stages) and 1.3e-5 (camera stage) here, above
    CLOSURE_GRAD_TOL: the whole-vector bound follows the block rule, max(CLOSURE_GRAD_TOL, 10 x the float32 oracle's
    whole-vector error); the loss stays at CLOSURE_LOSS_TOL."""
    label = "near-%s-%s" % (which, mode)
    dev = device_closures(synth_model, which, "near", mode)
    for stage, (loss, grad) in sorted(dev.items()):
        lo, go, go32, blocks = oracle_closures(synth_model, which, "near", stage)
        H.assert_blocks_tile(blocks, grad.shape[1])
        whole = max(H.closure_errors(0.0, 1.0, go32[i], go[i])[1] for i in range(len(lo)))
        for i in range(len(lo)):
            H.check_closure(label, stage, loss[i], lo[i], grad[i], go[i], grad_tol=max(H.CLOSURE_GRAD_TOL, 10.0 * whole))
        H.check_closure_blocks(label, stage, grad, go, go32, blocks)


@pytest.mark.parametrize("pts", ["far", "near"])
@pytest.mark.parametrize("which", ["body", "full", "halpe", "vposer"])
def test_dense_and_rows_agree_per_block(gpu, synth_model, which, pts):
    """Set (c): the dense path's gradient against the needed-rows path's at the same points, every block under the bound that
    block has against the oracle (test_dense_and_rows_agree_per_closure compares the whole norm only)."""
    rows, dense = device_closures(synth_model, which, pts, "rows"), device_closures(synth_model, which, pts, "dense")
    assert sorted(rows) == sorted(dense)
    for stage in sorted(rows):
        _, go, go32, blocks = oracle_closures(synth_model, which, pts, stage)
        H.check_closure_blocks("rows-vs-dense-%s-%s" % (pts, which), stage, dense[stage][1], rows[stage][1], None, blocks,
                               yardstick=H.block_yardstick(go, go32, blocks))
