"""Self-served blend offsets in the dense loop (run with -m gpu).  In rounds of the third form (csrc/host/fit_loop.hip DenseLoop::round_self) the tick
workgroup no longer reads the blend offsets of its keypoint vertices from the dense GEMM's export (BatchDev.uvp): it forms them
itself from its operand row with the GEMM's own chain of fp32 operations (csrc/closure_lds.h self_blend_offsets), and the whole
GEMM of every evaluation runs beside the tick chain.  Nobody's arithmetic changes, so every comparison here is bit for bit:
the routine against the GEMM's export, the loops against each other, a frame of a job against the frame alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import test_gpu_parity as T
import test_gpu_dense_overlap as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cfg_body():
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg["use_camera_prior"] = False
    return cfg


def _posed_batch(dm, cfg, frames, B, seed, nemb):
    """B frames (i % 3 of the synthetic set) at B different random points: poses, shapes and expressions all differ."""
    fb = H.engine_batch_from_frames(dm, cfg, frames, [i % 3 for i in range(B)], lbs_mode="dense")
    rng = np.random.RandomState(seed)
    P = H.random_params(rng, B, scale=0.5)
    P["pose_embedding"] = (0.3 * rng.normal(size=(B, nemb))).astype(np.float32)
    P["cam_translation"] = np.tile(np.array([[0.0, 0.0, 3.0]], np.float32), (B, 1))
    fb.set_params(**P)
    return fb


def _check_routine(fb, dm, B, stages):
    for stage in stages:
        fb.closure(stage)
        gemm, own = fb.debug_read("uvp"), fb.debug_read("uvp_self")
        assert gemm.shape == own.shape == (B, dm.n_uniq * 3)
        assert np.array_equal(own, gemm), (stage, B, np.abs(own - gemm).max())
        if dm.n_uniq:
            assert np.abs(gemm).max() > 0
            if B > 1:       # the frames carry different poses: so do their offsets
                assert not np.array_equal(gemm[0], gemm[1])


@pytest.mark.parametrize("B", [1, 17, 33])
def test_self_served_offsets_equal_the_gemm_export_body_only(synth_model, cfg_body, B):
    """The body-only joint map: 11 exported vertices, one partial tile.  B = 1 and 17 go through k_lbs_dense16c (one and two
    16-frame slices), 33 through k_lbs_dense16<4>; after a closure at the camera stage and at the first body stage,
    debug_read("uvp_self") -- the routine on the current operand rows -- equals debug_read("uvp"), what the GEMM wrote."""
    dm = T._dm(synth_model, cfg_body)
    assert dm.n_uniq == 11
    fb = _posed_batch(dm, cfg_body, T.synth_frames(synth_model, cfg_body, 3), B, 11 + B, 63)
    _check_routine(fb, dm, B, (-1, 0))
    fb.close()


def test_self_served_offsets_of_a_model_without_vertex_keypoints_are_empty(synth_model, cfg_body):
    """The joint map of test_a_batch_without_vertex_keypoints_fits: every keypoint is a kinematic joint, n_uniq = 0.  Both arrays
    are empty and nothing is launched for them."""
    from smplifyx_amd import engine
    jm = np.array(H.joint_map_for(cfg_body)).copy()
    jm[jm >= 55] = np.where(np.arange(len(jm))[jm >= 55] < 19, 15, 7)
    dm = engine.DeviceModel(synth_model, joint_map=jm, num_betas=cfg_body["num_betas"],
                            num_expression_coeffs=cfg_body["num_expression_coeffs"],
                            num_pca_comps=cfg_body["num_pca_comps"], use_face_contour=cfg_body["use_face_contour"])
    assert dm.n_uniq == 0
    fb = _posed_batch(dm, cfg_body, T.synth_frames(synth_model, cfg_body, 3), 3, 5, 63)
    _check_routine(fb, dm, 3, (-1, 0))
    fb.close()
    dm.close()


def test_self_served_offsets_equal_the_gemm_export_hands_and_face(synth_model):
    """The hands + face joint map of fit_smplx_smplifyx.yaml (extra vertices, static landmarks, every corner a dynamic-contour
    landmark can land on): several tiles of exported vertices, the last one partial, dealt to the routine's wavefronts in turn."""
    from smplifyx_amd import synthetic
    cfg = H.load_cfg("fit_smplx_smplifyx.yaml")
    dm = T._dm(synth_model, cfg, vposer=synthetic.make_synthetic_vposer(0))
    assert dm.n_uniq > 16 and dm.n_uniq % 16 != 0, dm.n_uniq
    frames = T.synth_frames(synth_model, cfg, 3)
    fb = _posed_batch(dm, cfg, frames, 2, 7, 32)
    _check_routine(fb, dm, 2, (-1, 0))
    fb.close()


@H.requires_lab()
def test_the_four_loops_give_the_same_bits():
    """The two jobs of test_gpu_dense_overlap._JOB (90 frames resident: compaction through every GEMM kernel down to the 16c tail;
    40 frames through slots=16: admission while a GEMM is in flight), each in a process of its own (the switches are read once)
    under: the shipped rule; SFX_OVERLAP_SERIAL=0, every round self-served down to one column; SFX_DENSE_SELF=0 with
    SFX_OVERLAP_SERIAL=16, the key / rest form above 16 columns; SFX_DENSE_OVERLAP=0, the serial whole-grid loop.  The sha256 over
    the fitted parameters, stage_evals, stage_loss and every row of debug_read("verts") must agree in all four."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = O._JOB % {"root": root, "tests": os.path.join(root, "tests")}
    settings = (("default", {}), ("self_all", {"SFX_OVERLAP_SERIAL": "0"}),
                ("key_rest16", {"SFX_DENSE_SELF": "0", "SFX_OVERLAP_SERIAL": "16"}), ("serial", {"SFX_DENSE_OVERLAP": "0"}))
    outs = {}
    for name, extra in settings:
        env = dict(os.environ)
        for k in ("SFX_DENSE_OVERLAP", "SFX_OVERLAP_SERIAL", "SFX_DENSE_SELF", "SFX_DENSE_SELF_MAX", "SFX_DENSE_SELF_SERIAL"):
            env.pop(k, None)
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        outs[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(outs)
    for name, _ in settings:
        assert outs[name]["resident90"]["evals"] > 90 * 50 and outs[name]["pooled40"]["evals"] > 40 * 50, (name, outs)
        assert outs[name] == outs["serial"], (name, outs)


def test_a_frame_of_24_equals_the_frame_alone(synth_model, cfg_body):
    """Whatever the shipped rule does at 24 active columns (and at the fewer left as frames finish): the 24-frame job i % 3
    against its three frames fitted alone -- parameters, stage losses and evaluation counts bit for bit."""
    dm = T._dm(synth_model, cfg_body)
    frames = T.synth_frames(synth_model, cfg_body, 3)
    alone = [O._fit(dm, cfg_body, frames, [t]) for t in range(3)]
    job = O._fit(dm, cfg_body, frames, [i % 3 for i in range(24)])
    assert job["stage_evals"].sum() > 24 * 50
    for i in range(24):
        a = alone[i % 3]
        for k in a["params"]:
            assert np.array_equal(job["params"][k][i], a["params"][k][0]), (i, k)
        assert np.array_equal(job["stage_loss"][i], a["stage_loss"][0]) and np.array_equal(job["stage_evals"][i], a["stage_evals"][0]), i
