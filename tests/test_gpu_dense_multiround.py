"""The multi-round form of the dense loop (run with -m gpu): at few active columns the ticks of up to eight rounds are one launch
whose workgroups loop over their frame's rounds (csrc/fused.hip k_tick_dense_multi), the GEMMs of those rounds run behind it on
the second stream, and the operand sets rotate through csrc/operand_ring.h (csrc/host/fit_loop.hip DenseLoop::launch_multi).
Nobody's arithmetic changes, so every comparison here is bit for bit: against the serial loop and the loop without the form
(lab build), against the same frame fitted alone, and against the same job run twice."""
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

_SWITCHES = ("SFX_DENSE_OVERLAP", "SFX_OVERLAP_SERIAL", "SFX_DENSE_SELF", "SFX_DENSE_SELF_MAX", "SFX_DENSE_MULTI", "SFX_DENSE_MULTI_MAX",
             "SFX_DENSE_MULTI_R", "SFX_POLL_ROUNDS", "SFX_POLL_AHEAD")


# The two jobs of test_gpu_dense_overlap._JOB -- the same frames, sizes and pools -- with the hash in two parts: "fit" over
# parameters, stage_evals and stage_loss, "sha" over those and every row of debug_read("verts").
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
    fit = h.hexdigest()
    h.update(np.ascontiguousarray(fb.debug_read("verts")).tobytes())
    out[name] = {"sha": h.hexdigest(), "fit": fit, "evals": int(np.asarray(st["stage_evals"]).sum())}
    fb.close()
print(json.dumps(out))
'''


def _run_jobs(switches):
    """The two jobs of test_gpu_dense_overlap._JOB -- 90 frames resident, compacting down to one column; 40 frames through
    slots=16, admitted between batches -- in a process of their own (the lab build reads its switches once)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(switches)
    r = subprocess.run([sys.executable, "-c", _JOB % {"root": root, "tests": os.path.join(root, "tests")}], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


_SERIAL = {}


@pytest.fixture(scope="module")
def serial_jobs():
    """The serial loop (SFX_DENSE_OVERLAP=0) at a polling cadence, run once per cadence."""
    def get(poll_rounds):
        if poll_rounds not in _SERIAL:
            _SERIAL[poll_rounds] = _run_jobs(dict({"SFX_DENSE_OVERLAP": "0"}, **({"SFX_POLL_ROUNDS": poll_rounds} if poll_rounds else {})))
        return _SERIAL[poll_rounds]
    return get


@H.requires_lab()
@pytest.mark.parametrize("name,switches", [
    ("shipped", {}),
    ("no-multi", {"SFX_DENSE_MULTI": "0"}),
    ("multi-everywhere", {"SFX_DENSE_MULTI_MAX": "256"}),
    ("one-round-launches", {"SFX_DENSE_MULTI_R": "1", "SFX_POLL_ROUNDS": "7"}),
    ("three-round-launches", {"SFX_DENSE_MULTI_R": "3", "SFX_POLL_ROUNDS": "7"}),
])
def test_the_loops_with_and_without_multi_round_launches_give_the_same_bits(serial_jobs, name, switches):
    """One sha256 over the fitted parameters, stage_evals, stage_loss and every row of debug_read("verts") -- the rows of finished
    frames included -- from the serial loop (SFX_DENSE_OVERLAP=0) and from: the shipped rule (multi-round launches at <= 96
    columns: both jobs all the way, the resident one through its compactions down to one column); the loop without the form
    (SFX_DENSE_MULTI=0: self-served rounds at 90 columns, serial ones from 64 down); every batch multi-round whatever the columns
    (SFX_DENSE_MULTI_MAX=256); launches of one and of
    three rounds in batches of seven (3 + 3 + 1: launch sizes that do not divide the batch, an odd walk through the ring).
    The rows of verts that a compaction drops keep the mesh of the last evaluation skinned before it, and WHEN the loop compacts
    follows the polling cadence, in the serial loop too: the runs with batches of seven are held, verts included, against the
    serial loop with batches of seven, and their parameters, stage_evals and stage_loss against the default serial loop's as well."""
    out = _run_jobs(switches)
    print(name, out)
    assert out["resident90"]["evals"] > 90 * 50 and out["pooled40"]["evals"] > 40 * 50, out
    ref = serial_jobs(switches.get("SFX_POLL_ROUNDS"))
    assert out == ref, (name, out, ref)
    base = serial_jobs(None)
    assert {k: (v["fit"], v["evals"]) for k, v in out.items()} == {k: (v["fit"], v["evals"]) for k, v in base.items()}, (name, out, base)


@pytest.fixture(scope="module")
def cfg_body():
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg["use_camera_prior"] = False
    return cfg


@pytest.fixture(scope="module")
def alone(synth_model, cfg_body):
    """Frames 0, 1 and 2 each fitted alone: one column, so every round of the product library is in a multi-round launch --
    every stage switch and the finish happen in the middle of one."""
    dm = T._dm(synth_model, cfg_body)
    frames = T.synth_frames(synth_model, cfg_body, 3)
    return [O._fit(dm, cfg_body, frames, [t]) for t in range(3)]


def test_seventeen_frames_equal_each_frame_alone(synth_model, cfg_body, alone):
    """17 frames as i % 3 (two 16-frame slices, then one) against each of the three fitted alone: parameters, stage_loss and
    stage_evals bit for bit.  Frames of one kind finish in the same round of the same launch, the kinds apart."""
    dm = T._dm(synth_model, cfg_body)
    frames = T.synth_frames(synth_model, cfg_body, 3)
    idx = [i % 3 for i in range(17)]
    b = O._fit(dm, cfg_body, frames, idx)
    assert min(int(a["stage_evals"][0].sum()) for a in alone) > 50
    for i, t in enumerate(idx):
        a = alone[t]
        for k in a["params"]:
            assert np.array_equal(b["params"][k][i], a["params"][k][0]), (i, k)
        assert np.array_equal(b["stage_loss"][i], a["stage_loss"][0]) and np.array_equal(b["stage_evals"][i], a["stage_evals"][0]), i


def test_the_same_job_twice_in_one_process_gives_the_same_bits(synth_model, cfg_body):
    """24 frames twice on one batch handle's worth of state each, in one process: the second fit starts on the ring position,
    the events and the second stream the first one left; verts included."""
    dm = T._dm(synth_model, cfg_body)
    frames = T.synth_frames(synth_model, cfg_body, 3)
    idx = [i % 3 for i in range(24)]
    fb = O._batch(dm, cfg_body, frames, idx)
    start = {k: v.copy() for k, v in fb.get_params().items() if k != "body_pose"}      # every parameter block as the batch was set up
    outs = []
    for _ in range(2):
        fb.set_params(regression_pose=frames["reg_pose"][idx], **start)
        fb.guess_init(cfg_body["body_tri_idxs"])
        fb.fit(first_stage=-1, last_stage=1)
        st = fb.stats()
        outs.append(dict(params={k: v.copy() for k, v in fb.get_params().items()}, stage_loss=st["stage_loss"].copy(),
                         stage_evals=st["stage_evals"].copy(), verts=fb.debug_read("verts").copy()))
    fb.close()
    a, b = outs
    assert int(a["stage_evals"].sum()) > 24 * 50
    for k in ("stage_loss", "stage_evals", "verts"):
        assert np.array_equal(a[k], b[k]), k
    for k in a["params"]:
        assert np.array_equal(a["params"][k], b["params"][k]), k
