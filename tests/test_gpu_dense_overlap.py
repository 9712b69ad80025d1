"""The overlapped dense loop (run with -m gpu): the GEMM's key tiles in front of the tick kernel, every other tile beside it on a
second stream, three sets of operand buffers (csrc/host/fit_loop.hip DenseLoop::round_key_rest).  Nobody's arithmetic changes, so every comparison here
is bit for bit: against the serial whole-grid loop (lab build, SFX_DENSE_OVERLAP=0), against the same frame fitted alone,
against the same job resident instead of pooled, and against itself run twice."""
import numpy as np
import pytest

import helpers as H
import test_gpu_parity as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cfg_body():
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg["use_camera_prior"] = False
    return cfg


def _batch(dm, cfg, frames, idx, slots=0):
    """H.engine_batch_from_frames (dense, entry evaluation reused) with a column pool."""
    from smplifyx_amd import engine
    idx = list(idx)
    B = len(idx)
    kp = frames["keypoints"][idx]
    K = kp.shape[1]
    jw = np.tile(H.base_joint_weights(cfg, K), (B, 1))
    cm = np.zeros((B, K), np.float32); cm[:, cfg["init_joints_idxs"]] = 1
    fb = engine.FrameBatch(dm, B, cfg, lbs_mode="dense", reuse_entry_eval=True, has_regression_pose=True, slots=slots)
    fb.set_frames(kp, jw, cm, frames["focal"], np.tile([frames["W"] * 0.5, frames["H"] * 0.5], (B, 1)), 1000.0 / frames["H"])
    fb.set_params(regression_pose=frames["reg_pose"][idx], global_orient=frames["reg_global"][idx],
                  pose_embedding=frames["reg_pose"][idx], cam_translation=np.zeros((B, 3), np.float32))
    return fb


_JOB = r'''
import hashlib, json, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import helpers as H, test_gpu_parity as T, test_gpu_dense_overlap as O
from smplifyx_amd import synthetic
model = synthetic.make_synthetic_model(0)
cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False); cfg["use_camera_prior"] = False
dm = T._dm(model, cfg)
frames = T.synth_frames(model, cfg, 5)
out = {}
for name, n, mod, slots in (("resident90", 90, 5, 0), ("pooled40", 40, 5, 16)):
    fb = O._batch(dm, cfg, frames, [i %% mod for i in range(n)], slots=slots)
    fb.guess_init(cfg["body_tri_idxs"])
    fb.fit(first_stage=-1, last_stage=1)
    P = fb.get_params(); st = fb.stats()
    h = hashlib.sha256()
    for k in sorted(P): h.update(np.ascontiguousarray(P[k]).tobytes())
    h.update(np.ascontiguousarray(st["stage_evals"]).tobytes()); h.update(np.ascontiguousarray(st["stage_loss"]).tobytes())
    h.update(np.ascontiguousarray(fb.debug_read("verts")).tobytes())
    out[name] = {"sha": h.hexdigest(), "evals": int(np.asarray(st["stage_evals"]).sum())}
    fb.close()
print(json.dumps(out))
'''


@H.requires_lab()
def test_overlapped_and_serial_loops_give_the_same_bits():
    """SFX_DENSE_OVERLAP=0 (lab build) selects the serial whole-grid loop.  Two jobs, each once per loop, in processes of their
    own (the switch is read once): 90 frames as i % 5 -- six slices, so k_lbs_dense16<3>, then <5>, <4> and the 16c tail as
    frames finish, with compaction on the way -- and 40 frames through slots=16, where frames are admitted while a rest-tile
    GEMM is in flight.  A sha256 over the fitted parameters, stage_evals, stage_loss and every row of debug_read("verts") (the
    rows of finished frames included: the stale-buffer hazard of several operand sets) must agree.  The loop's own rule
    overlaps rounds at more than 160 active columns only, which these jobs never have: they run a third time with
    SFX_OVERLAP_SERIAL=16, which overlaps every round above 16 columns -- that run is the one that covers the protocol."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _JOB % {"root": root, "tests": os.path.join(root, "tests")}
    outs = {}
    for name, val, thr in (("overlap", None, None), ("overlap16", None, "16"), ("serial", "0", None)):
        env = dict(os.environ)
        env.pop("SFX_DENSE_OVERLAP", None); env.pop("SFX_OVERLAP_SERIAL", None)
        if val is not None:
            env["SFX_DENSE_OVERLAP"] = val
        if thr is not None:
            env["SFX_OVERLAP_SERIAL"] = thr
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(outs)
    assert outs["overlap"]["resident90"]["evals"] > 90 * 50 and outs["overlap"]["pooled40"]["evals"] > 40 * 50, outs
    assert outs["overlap"] == outs["serial"] and outs["overlap16"] == outs["serial"], outs


def _fit(dm, cfg, frames, idx, slots=0):
    fb = _batch(dm, cfg, frames, idx, slots=slots)
    fb.guess_init(cfg["body_tri_idxs"])
    l, g = fb.closure(0)
    fb.fit(first_stage=-1, last_stage=1)
    n = len(idx)
    out = dict(loss=l.copy(), grad=g.copy(), params={k: v.copy() for k, v in fb.get_params().items()},
               stage_loss=fb.stats()["stage_loss"].copy(), stage_evals=fb.stats()["stage_evals"].copy(),
               verts=fb.debug_read("verts").reshape(n, -1).copy())
    fb.close()
    return out


@pytest.fixture(scope="module")
def alone(synth_model, cfg_body):
    """Frames 0, 1 and 2 each fitted alone."""
    dm = T._dm(synth_model, cfg_body)
    frames = T.synth_frames(synth_model, cfg_body, 3)
    return [_fit(dm, cfg_body, frames, [t]) for t in range(3)]


# 40 frames: the size the loop's rule keeps serial (<= 160 active columns); 200: rounds of the product library that overlap
@pytest.fixture(scope="module", params=[40, 200])
def jobs(request, synth_model, cfg_body, alone):
    """The B-frame job (0, 1, 0, 1, ..., 2) twice in this process, next to its three frames fitted alone."""
    dm = T._dm(synth_model, cfg_body)
    frames = T.synth_frames(synth_model, cfg_body, 3)
    idx = [i % 2 for i in range(request.param - 1)] + [2]
    return dict(idx=idx, alone=alone, batch=[_fit(dm, cfg_body, frames, idx) for _ in range(2)])


def test_a_frame_in_a_batch_equals_the_frame_alone(jobs):
    """Frame 2 alone against frame 2 as the last of B whose others finish at other rounds: entry loss and gradient, fitted
    parameters, stage losses and evaluation counts bit for bit -- and so for every other frame of the batch against its own
    fit alone."""
    b, idx = jobs["batch"][0], jobs["idx"]
    for i, t in enumerate(idx):
        a = jobs["alone"][t]
        assert b["loss"][i] == a["loss"][0] and np.array_equal(b["grad"][i], a["grad"][0]), i
        for k in a["params"]:
            assert np.array_equal(b["params"][k][i], a["params"][k][0]), (i, k)
        assert np.array_equal(b["stage_loss"][i], a["stage_loss"][0]) and np.array_equal(b["stage_evals"][i], a["stage_evals"][0]), i


def test_finished_frames_keep_the_mesh_of_their_last_evaluation(jobs):
    """The stale-buffer hazard.  A frame that has finished exports no more, while the GEMMs go on recomputing its column for as
    long as the host's decisions lag (up to 32 rounds): with several operand sets the column would cycle through the operands
    of its last evaluations unless its workgroup leaves all sets equal.  After the fit, a row of
    debug_read("verts") that belonged to one frame from its first evaluation to the end must be the row of the same frame fitted
    alone, bit for bit.  Which rows those are follows from the loop's rules: rows are GEMM columns; of frames 0 / 1 (the
    alternating ones) the kind with fewer evaluations finishes first, the first compaction then packs the at most B / 2 + 1
    frames still running into rows 0 .. B / 2, and the rows from B / 2 + 2 up of the kind that finished first are never written
    again (40 frames: rows 22 and up).  Row 0 of the batch ends as the last mesh of whichever frame sat there last.  At 200
    frames the first kind finishes in overlapped rounds (200 active columns)."""
    b, alone, B = jobs["batch"][0], jobs["alone"], len(jobs["idx"])
    ev = [int(a["stage_evals"][0].sum()) for a in alone]
    print("evaluations of frames 0 / 1 / 2 fitted alone:", ev)
    assert abs(ev[0] - ev[1]) > 64, "the two kinds must finish more than the polling lag apart for this test's reasoning"
    first = 0 if ev[0] < ev[1] else 1
    rows = [r for r in range(B // 2 + 2, B - 1) if r % 2 == first]
    assert len(rows) >= 8
    for r in rows:
        assert np.array_equal(b["verts"][r], alone[first]["verts"][0]), r
    assert any(np.array_equal(b["verts"][0], a["verts"][0]) for a in alone)
    assert np.abs(alone[first]["verts"][0]).max() > 0.1
    if ev[2] < min(ev[0], ev[1]):          # frame 2 finished before the first compaction: the last row stayed its own
        assert np.array_equal(b["verts"][B - 1], alone[2]["verts"][0])


def test_the_same_job_twice_in_one_process_gives_the_same_bits(jobs):
    """The second fit starts with the operand buffers, events and second stream the first one left behind."""
    a, b = jobs["batch"]
    for k in ("loss", "grad", "stage_loss", "stage_evals", "verts"):
        assert np.array_equal(a[k], b[k]), k
    for k in a["params"]:
        assert np.array_equal(a["params"][k], b["params"][k]), k


@pytest.mark.parametrize("B,slots", [(48, 16), (240, 192)])
def test_a_pooled_job_equals_the_resident_one(synth_model, cfg_body, B, slots):
    """48 frames through slots=16 (a pool of 32 columns: 16 frames wait and are admitted into the columns of finished ones) and
    240 through slots=192 (a pool the loop's rule overlaps: frames are admitted while rest-tile GEMMs are in flight) against
    the same frames resident: stage_loss and parameters bit for bit."""
    dm = T._dm(synth_model, cfg_body)
    frames = T.synth_frames(synth_model, cfg_body, 3)
    idx = [i % 3 for i in range(B)]
    res, pool = _fit(dm, cfg_body, frames, idx), _fit(dm, cfg_body, frames, idx, slots=slots)
    assert np.all(np.isfinite(res["stage_loss"][:, :3]))
    assert np.array_equal(res["stage_loss"], pool["stage_loss"]) and np.array_equal(res["stage_evals"], pool["stage_evals"])
    for k in res["params"]:
        assert np.array_equal(res["params"][k], pool["params"][k]), k


@pytest.mark.parametrize("B", [40, 200])
def test_a_batch_without_vertex_keypoints_fits(synth_model, cfg_body, B):
    """The empty key list: a joint map whose 25 keypoints are all kinematic joints (the face and foot keypoints of the COCO-25
    map, which are vertices of the mesh, replaced by the head and ankle joints) exports no vertex, so the loop launches no key
    tiles and the tick kernel waits for nothing of the GEMM (200 frames: rounds that overlap).  The batch must fit, and a
    frame of it must equal itself alone."""
    from smplifyx_amd import engine
    jm = np.array(H.joint_map_for(cfg_body)).copy()
    assert (jm >= 55).any()
    jm[jm >= 55] = np.where(np.arange(len(jm))[jm >= 55] < 19, 15, 7)
    dm = engine.DeviceModel(synth_model, joint_map=jm, num_betas=cfg_body["num_betas"],
                            num_expression_coeffs=cfg_body["num_expression_coeffs"],
                            num_pca_comps=cfg_body["num_pca_comps"], use_face_contour=cfg_body["use_face_contour"])
    frames = T.synth_frames(synth_model, cfg_body, 3)
    idx = [i % 2 for i in range(B - 1)] + [2]
    alone, batch = _fit(dm, cfg_body, frames, [2]), _fit(dm, cfg_body, frames, idx)
    sl = batch["stage_loss"][:, :3]
    assert np.all(np.isfinite(sl)) and np.all(sl[:, 1] < batch["loss"]) and batch["stage_evals"].sum() > B * 50
    assert np.array_equal(batch["stage_loss"][-1], alone["stage_loss"][0])
    for k in alone["params"]:
        assert np.array_equal(batch["params"][k][-1], alone["params"][k][0]), k
    dm.close()
