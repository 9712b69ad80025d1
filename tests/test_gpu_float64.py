"""The float64 mode (sfx_batch_cfg.high_precision = 2, FrameBatch(precision="float64")) on the MI355X: the closure in double
against fp64 autograd of the oracle, its batch invariance, and the refusals of the C ABI between float and float64 batches."""
import os

import numpy as np
import pytest
import torch

import helpers as H
import test_gpu_parity as T
from test_gpu_parity import gpu      # noqa: F401  (the GPU fixture of the parity tests)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# bounds about 10x the maxima observed on the MI355X: loss 6.8e-16, gradient 1.2e-15 relative (the fp32 closure sits at
# 1.9e-7 / 3.7e-7)
LOSS_TOL, GRAD_TOL = 1e-14, 1e-14


@pytest.fixture(scope="module")
def cfg64():
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg.update(float_dtype="float64")
    return cfg


def _batch(dm, cfg, frames, idx, precision="float64"):
    """A rows-mode FrameBatch of frames[idx] prepared as helpers.engine_batch_from_frames prepares one (regression prior)."""
    from smplifyx_amd import engine
    idx = list(idx)
    B = len(idx)
    kp = frames["keypoints"][idx]
    fb = engine.FrameBatch(dm, B, cfg, lbs_mode="rows", reuse_entry_eval=False, has_regression_pose=True, precision=precision)
    fb.set_frames(kp, T._jw(cfg, dict(keypoints=kp)), T._cmask(cfg, dict(keypoints=kp)), frames["focal"],
                  np.tile([frames["W"] * 0.5, frames["H"] * 0.5], (B, 1)), 1000.0 / frames["H"])
    fb.set_params(regression_pose=frames["reg_pose"][idx], global_orient=frames["reg_global"][idx],
                  pose_embedding=frames["reg_pose"][idx], cam_translation=np.zeros((B, 3), np.float32))
    return fb


def _e2e_frames(dm, cfg):
    """The two frames of tests/golden/e2e_synth.npz (800 x 600 image, focal 5000) with cam_t from the fp32 batch's guess_init."""
    g = np.load(os.path.join(GOLD, "e2e_synth.npz"))
    frames = dict(keypoints=g["keypoints"], reg_pose=g["reg_pose"], reg_global=g["reg_global"], H=600, W=800, focal=5000.0)
    fb = _batch(dm, dict(cfg, float_dtype="float32"), frames, range(2), precision="mixed")
    fb.guess_init(cfg["body_tri_idxs"])
    frames["cam_t"] = fb.get_params()["cam_translation"].astype(np.float64)
    fb.close()
    return frames


def _probe(model, dm, cfg, frames, label, seed):
    """closure_f64 against the oracle's fp64 autograd at seeded points near the frames' regression poses."""
    B = frames["keypoints"].shape[0]
    fb = _batch(dm, cfg, frames, range(B))
    assert fb.float64
    rng = np.random.RandomState(seed)
    P = H.random_params(rng, B, scale=0.5)
    P["pose_embedding"] = frames["reg_pose"] + 0.1 * rng.normal(size=(B, 63)).astype(np.float32)
    P["global_orient"] = frames["reg_global"] + 0.1 * rng.normal(size=(B, 3)).astype(np.float32)
    P["cam_translation"] = (frames["cam_t"] + 0.3 * rng.normal(size=(B, 3))).astype(np.float32)
    est = (frames["cam_t"][:, 2] + 1.0).astype(np.float32)
    fb.set_frames(frames["keypoints"], T._jw(cfg, frames), T._cmask(cfg, frames), frames["focal"],
                  np.tile([frames["W"] * 0.5, frames["H"] * 0.5], (B, 1)), 1000.0 / frames["H"], est_tz=est)
    fb.set_params(regression_pose=frames["reg_pose"], **P)
    P["est_tz"] = est
    got = fb.get_params()
    assert got["cam_translation"].dtype == np.float64
    np.testing.assert_array_equal(got["betas"], P["betas"].astype(np.float64))
    for stage in [-1] + list(range(fb.n_stages)):
        loss, grad = fb.closure(stage)
        assert loss.dtype == np.float64 and grad.dtype == np.float64
        np.testing.assert_array_equal(fb.last_grad(stage), grad)
        ref = []
        for i in range(B):
            lo, go, go32, blocks = T._oracle_closure_blocks(model, cfg, frames, i, P, stage)
            ref.append((go, go32))
            H.check_closure(label, stage, loss[i], lo, grad[i], go, loss_tol=LOSS_TOL, grad_tol=GRAD_TOL)
            if stage >= 0:
                assert np.all(grad[i][13:13 + 63] == 0)      # the dead body_pose parameter
        # every parameter block: the float32 oracle's own error in the block, scaled to float64's unit roundoff
        H.assert_blocks_tile(blocks, fb.num_vars(stage))
        H.check_closure_blocks(label, stage, grad, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), blocks,
                               floor=GRAD_TOL, unit_ratio=H.F64_UNIT_RATIO)
    fb.close()


def test_float64_closure_matches_fp64_oracle(gpu, synth_model, cfg64):
    """Loss and gradient of sfx_batch_closure_f64 against fp64 autograd of the oracle, camera stage and every body stage:
    3 synthetic frames and the 2 frames of e2e_synth."""
    dm = T._dm(synth_model, cfg64)
    _probe(synth_model, dm, cfg64, T.synth_frames(synth_model, cfg64, 3), "f64-body-rows-synth", 11)
    _probe(synth_model, dm, cfg64, _e2e_frames(dm, cfg64), "f64-body-rows-e2e", 12)
    dm.close()


def test_float64_closure_is_batch_invariant(gpu, synth_model, cfg64):
    """Frames evaluated alone or inside a batch of 64 give the same bits (fixed summation orders, DPP in f64)."""
    dm = T._dm(synth_model, cfg64)
    frames = T.synth_frames(synth_model, cfg64, 64)
    rng = np.random.RandomState(3)
    P = H.random_params(rng, 64, scale=0.5)
    P["pose_embedding"] = frames["reg_pose"] + 0.1 * rng.normal(size=(64, 63)).astype(np.float32)
    P["cam_translation"] = frames["cam_t"].astype(np.float32)
    stages = [-1] + list(range(3))
    fb = _batch(dm, cfg64, frames, range(64))
    fb.set_params(**P)
    full = [fb.closure(s) for s in stages]
    fb.close()
    for i in (0, 17, 63):
        fb = _batch(dm, cfg64, frames, [i])
        fb.set_params(**{k: v[i:i + 1] for k, v in P.items()})
        for s, (l64, g64) in zip(stages, full):
            l1, g1 = fb.closure(s)
            assert l64[i] == l1[0] and np.array_equal(g64[i], g1[0]), (i, s)
        fb.close()
    dm.close()


def test_float64_and_float_batches_refuse_each_others_outputs(gpu, synth_model, cfg64):
    from smplifyx_amd import _capi, engine
    dm = T._dm(synth_model, cfg64)
    frames = T.synth_frames(synth_model, cfg64, 2)
    fb64 = _batch(dm, cfg64, frames, range(2))
    lib = fb64._lib
    f = np.zeros((2, 256), np.float32)
    with pytest.raises(_capi.SfxError, match="float64"):
        _capi.check(lib.sfx_batch_closure(fb64._h, 0, _capi.fptr(f[:, 0].copy()), None, None))
    with pytest.raises(_capi.SfxError, match="float64"):
        _capi.check(lib.sfx_batch_get_params(fb64._h, *([_capi.fptr(f)] * 11)))
    with pytest.raises(_capi.SfxError, match="float64"):
        fb64.fit()
    with pytest.raises(_capi.SfxError, match="float64"):
        fb64.guess_init(cfg64["body_tri_idxs"])
    with pytest.raises(_capi.SfxError, match="float64"):
        fb64.get_trace()
    with pytest.raises(_capi.SfxError):
        _capi.check(lib.sfx_batch_set_gmm(fb64._h, 1, 63, _capi.fptr(f), _capi.fptr(f), _capi.fptr(f)))
    fb64.close()
    fb32 = _batch(dm, cfg64, frames, range(2), precision="mixed")
    assert not fb32.float64
    d = np.zeros((2, 256), np.float64)
    with pytest.raises(_capi.SfxError, match="not in float64 mode"):
        _capi.check(lib.sfx_batch_closure_f64(fb32._h, 0, _capi.dptr(d[:, 0].copy()), None, None))
    with pytest.raises(_capi.SfxError, match="not in float64 mode"):
        _capi.check(lib.sfx_batch_get_params_f64(fb32._h, *([_capi.dptr(d)] * 11)))
    fb32.close()
    with pytest.raises(ValueError, match="lbs_mode"):
        engine.FrameBatch(dm, 2, cfg64, lbs_mode="dense", has_regression_pose=True, precision="float64")
    dm.close()
