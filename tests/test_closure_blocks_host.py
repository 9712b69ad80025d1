"""The per-block gradient check (helpers.gradient_blocks / block_errors / check_closure_blocks) tested on the CPU, with the
float64 oracle gradient at point sets (a) (far) and (b) (near the solution) of the full coco25 cfg and the VPoser cfg:
the float32 oracle put in the device's place passes every block; an error of 1e-3 planted in one small block passes the
whole-vector check_closure and fails the block check, naming the block; the blocks agree with the engine's parameter list."""
import numpy as np
import pytest

import helpers as H
import test_gpu_closure_blocks as C

CASES = [("full", "far", (-1, 0, 1, 2)), ("full", "near", (-1, 0, 1, 2)), ("vposer", "far", (-1, 0, 3, 4)), ("vposer", "near", (-1, 0, 1, 2, 3, 4))]


def _logs():
    return dict(H.PARITY_LOG), dict(H.BLOCK_LOG)


def _restore(saved):
    for log, old in zip((H.PARITY_LOG, H.BLOCK_LOG), saved):
        log.clear(); log.update(old)


@pytest.mark.parametrize("which,pts,stages", CASES, ids=["%s-%s" % c[:2] for c in CASES])
def test_float32_oracle_passes_every_block(synth_model, which, pts, stages):
    cfg = C._cfg(which)
    for stage in stages:
        lo, go, go32, blocks = C.oracle_closures(synth_model, which, pts, stage)
        n = 6 if stage < 0 else (88 if cfg["use_vposer"] else 182)
        assert go.shape[1] == n
        H.assert_blocks_tile(blocks, n)
        saved = _logs()
        try:
            got = H.check_closure_blocks("host-f32-oracle-%s-%s" % (pts, which), stage, go32, go, go32, blocks)
        finally:
            _restore(saved)           # (the session summary is for device measurements)
        assert sorted(got) == sorted(b[0] for b in blocks)          # every block was looked at ...
        dead = [name for name, (err, share, bound) in got.items() if err is None]
        assert dead == (["body_pose"] if stage >= 0 and not cfg["use_vposer"] else [])     # ... and only the dead one without a ratio
        for i in range(go.shape[0]):
            assert [name for name, err, _ in H.block_errors(go32[i], go[i], blocks) if err is None] == dead
        # the bound of each block is the rule's: the floor, or 10 x the float32 oracle's own error (which therefore sits at
        # a tenth of it or less)
        y = H.block_yardstick(go, go32, blocks)
        for name, (err, share, bound) in got.items():
            if err is not None:
                assert bound == max(H.CLOSURE_GRAD_TOL, 10 * y[name]) and err == y[name] and err <= bound


def test_dead_block_must_be_exactly_zero(synth_model):
    lo, go, go32, blocks = C.oracle_closures(synth_model, "full", "far", 0)
    (a, b), = [(a, b) for name, a, b in blocks if name == "body_pose"]
    assert np.all(go[:, a:b] == 0) and np.all(go32[:, a:b] == 0)
    g = go32.copy(); g[1, a + 5] = 1e-30
    saved = _logs()
    try:
        with pytest.raises(AssertionError, match="dead block is not exactly zero.*body_pose"):
            H.check_closure_blocks("host-dead", 0, g, go, go32, blocks)
    finally:
        _restore(saved)


PLANTED = [("full", "betas"), ("full", "left_hand_pose"), ("full", "expression"), ("full", "leye_pose"), ("vposer", "pose_embedding")]


@pytest.mark.parametrize("which,block", PLANTED, ids=["%s-%s" % p for p in PLANTED])
def test_planted_block_error_passes_the_whole_norm_and_fails_the_block_check(synth_model, which, block):
    """Stage 0 at the far points (closure_probe's own / the VPoser test's own): one block of the float32 oracle's gradient
    scaled by 1 + 1e-3.  The jaw prior carries the norm there, so check_closure does not see it; check_closure_blocks does."""
    lo, go, go32, blocks = C.oracle_closures(synth_model, which, "far", 0)
    (a, b), = [(a, b) for name, a, b in blocks if name == block]
    g = go32.copy()
    g[:, a:b] *= 1.0 + 1e-3
    saved = _logs()
    try:
        # today's check passes where the block's share of the norm is below CLOSURE_GRAD_TOL / 1e-3 = 6e-3: in the frame in
        # which the block weighs least (every frame but one of the VPoser set, whose latent reaches a share of 7e-3)
        shares = [dict((n, sh) for n, _, sh in H.block_errors(go[i], go[i], blocks))[block] for i in range(go.shape[0])]
        quiet = [i for i in range(go.shape[0]) if shares[i] < 5e-3]
        assert int(np.argmin(shares)) in quiet and (which == "vposer" or len(quiet) == go.shape[0]), shares
        for i in quiet:
            le, ge = H.check_closure("host-planted", 0, lo[i], lo[i], g[i], go[i])
            assert ge <= H.CLOSURE_GRAD_TOL
        with pytest.raises(AssertionError) as ei:
            H.check_closure_blocks("host-planted", 0, g, go, go32, blocks)
        bad = ei.value.args[0][2]
        assert bad and all(item[0] == "closure gradient block" and item[1] == block for item in bad), bad
        assert len(bad) == go.shape[0]                                # in every frame
        # and nothing else in the vector is disturbed by the planted error
        others = [(n, a2, b2) for n, a2, b2 in blocks if n != block]
        for i in range(go.shape[0]):
            errs = dict((n, e) for n, e, _ in H.block_errors(g[i], go[i], blocks))
            assert abs(errs[block] - 1e-3) < 1e-4
            assert all(errs[n] == e for n, e, _ in H.block_errors(go32[i], go[i], blocks) if n != block)
    finally:
        _restore(saved)


@pytest.mark.parametrize("which", ["full", "pca-off", "vposer"])
def test_gradient_blocks_agree_with_the_engine_parameter_list(synth_model, which):
    """Names and sizes of the blocks against engine.PARAM_NAMES and the sizes FrameBatch.set_params / get_params use, PCA on, PCA
    off and with the VPoser latent.  The body stages of the reference order its variables as the body model registers them (not as
    PARAM_NAMES lists them) and end with pose_embedding; the camera stage is PARAM_NAMES[:2]."""
    import torch
    from oracle.body_model import SMPLXRef
    from smplifyx_amd import engine
    import test_gpu_parity as T
    cfg = C._cfg("vposer" if which == "vposer" else "full")
    npca = 45 if which == "pca-off" else cfg["num_pca_comps"]
    nemb = cfg.get("vposer_latent_dim", 32) if cfg["use_vposer"] else 63
    sizes = dict(cam_translation=3, global_orient=3, betas=cfg["num_betas"], left_hand_pose=npca, right_hand_pose=npca,
                 expression=cfg["num_expression_coeffs"], jaw_pose=3, leye_pose=3, reye_pose=3, pose_embedding=nemb)
    assert sorted(sizes) == sorted(engine.PARAM_NAMES)
    frames = T.synth_frames(synth_model, cfg, 3)
    orig = H.oracle_model
    if which == "pca-off":
        H.oracle_model = lambda model, cfg_, dtype=torch.float32: SMPLXRef(
            model, joint_map=H.joint_map_for(cfg_), num_betas=cfg_["num_betas"], num_expression_coeffs=cfg_["num_expression_coeffs"],
            use_pca=False, use_face_contour=cfg_["use_face_contour"], create_body_pose=True, dtype=dtype)
    try:
        ff = H.oracle_frame_fit(synth_model, cfg, frames, 0, dtype=torch.float64)
    finally:
        H.oracle_model = orig
    cam = H.gradient_blocks(ff, -1)
    assert [(n, b - a) for n, a, b in cam] == [(n, sizes[n]) for n in engine.PARAM_NAMES[:2]]
    H.assert_blocks_tile(cam, 6)
    body = H.gradient_blocks(ff, 0)
    assert body == H.gradient_blocks(ff, len(ff.stages) - 1)
    live = [(n, b - a) for n, a, b in body if n != "body_pose"]
    # every engine parameter but the camera's is one block, with the engine's size, and pose_embedding is the last one
    assert sorted(n for n, _ in live) == sorted(engine.PARAM_NAMES[1:]) and live[-1][0] == "pose_embedding"
    assert all(sz == sizes[n] for n, sz in live)
    # the body model's registration order (smplx.SMPL / SMPLH / SMPLX.__init__), which the device's variable table follows
    assert [n for n, _ in live] == ["betas", "global_orient", "left_hand_pose", "right_hand_pose", "jaw_pose", "leye_pose", "reye_pose",
                                    "expression", "pose_embedding"]
    dead = [(n, a, b) for n, a, b in body if n == "body_pose"]
    assert dead == ([] if cfg["use_vposer"] else [("body_pose", 13, 76)])
    total = sum(sz for _, sz in live) + (0 if cfg["use_vposer"] else 63)
    H.assert_blocks_tile(body, total)
    assert total == {"full": 182, "pca-off": 248, "vposer": 88}[which]
    if which == "pca-off":        # the device vector leaves the dead block out (test_use_pca_false_closure_matches_oracle)
        kept, keep = H.without_block(body, "body_pose")
        H.assert_blocks_tile(kept, 185)
        assert np.array_equal(keep, np.r_[0:13, 76:248])
