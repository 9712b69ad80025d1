"""A frame's state between the rounds of one multi-round tick launch (run with -m gpu).  From its second round on a workgroup of
csrc/fused.hip k_tick_dense_multi takes the forward state of the pending evaluation from LDS, where its own export pass left
it, and the optimiser's working set from where its own tick left it; only the first round of a launch reads them from global
memory, only the last export of a launch (or a frame's finish) saves the forward state to BatchDev.fwd, and every tick still
writes its working set back.  Nobody's arithmetic changes, so every comparison here is bit for bit: against the serial loop
and the loop without the form (lab build), against the same frame fitted alone, a smaller batch, and the same job run twice.

The jobs are short fits (maxiters = 8, stages -1 .. 1, about 180 evaluations per frame) of eight synthetic frames whose
evaluation counts put stage switches and finishes in the first, a middle and the last round of a launch -- asserted below from
stage_evals, for every launch length run."""
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
_MAXITERS = 8
_KINDS = 8                                   # synthetic frames 0 .. 7
_IDX17 = [i % _KINDS for i in range(17)]     # two 16-frame slices
_POLL = 7                                    # rounds per polled batch in the runs that vary the launch length
_R_MAX = 8                                   # SFX_TICK_ROUNDS: the longest launch

# Floats of a frame's row of BatchDev.fwd that an export pass defines (closure_lds.h FrameLDSBase up to `vp`, then the hand poses
# and the LUT row): feat | x[0 .. npar) | full_pose[0 .. 165) | R | Jr | G | A | Ad (fp64) | Gt (165 of 168 fp64) | lh45 rh45 lut_row.
# The rest of a row (the tail of x, padding) is whatever the LDS of the frame's first export held.
_FWD_N = 6016


def _fwd_defined(cfg):
    assert not cfg.get("use_vposer")
    npar = 6 + cfg["num_betas"] + 2 * cfg["num_pca_comps"] + cfg["num_expression_coeffs"] + 9 + 63 + 63      # host/batch.hip build_layout
    m = np.zeros(_FWD_N, bool)
    for a, n in ((0, 512), (512, npar), (768, 165), (936, 495 + 165 + 660 + 660), (2916, 1320), (4236, 330), (4572, 91)):
        m[a:a + n] = True
    return m


# 17 frames resident and 40 frames (i % 5) through slots = 16 -- admission and compaction between launches: the first round
# after an admission reads what tick_admit wrote -- in one process.  Per job: "fit" = sha256 over parameters, stage_evals and
# stage_loss, "sha" = over those and every row of debug_read("verts"), "fwd" = over the defined floats of debug_read "fwd".
_JOB = r'''
import hashlib, json, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import helpers as H, test_gpu_parity as T, test_gpu_dense_overlap as O, test_gpu_dense_multistate as S
from smplifyx_amd import synthetic, _capi as capi
model = synthetic.make_synthetic_model(0)
cfg = S._cfg()
dm = T._dm(model, cfg)
frames = T.synth_frames(model, cfg, S._KINDS)
mask = S._fwd_defined(cfg)
out = {}
for name, idx, slots in (("slices17", S._IDX17, 0), ("pooled40", [i %% 5 for i in range(40)], 16)):
    fb = O._batch(dm, cfg, frames, idx, slots=slots)
    fb.guess_init(cfg["body_tri_idxs"])
    fb.fit(first_stage=-1, last_stage=1)
    P = fb.get_params(); st = fb.stats()
    h = hashlib.sha256()
    for k in sorted(P): h.update(np.ascontiguousarray(P[k]).tobytes())
    h.update(np.ascontiguousarray(st["stage_evals"]).tobytes()); h.update(np.ascontiguousarray(st["stage_loss"]).tobytes())
    fit = h.hexdigest()
    h.update(np.ascontiguousarray(fb.debug_read("verts")).tobytes())
    fwd = np.zeros((len(idx), S._FWD_N), np.float32)
    capi.check(fb._lib.sfx_batch_debug_read(fb._h, b"fwd", capi.fptr(fwd), fwd.size))
    assert np.abs(fwd[:, :512]).max() > 0
    out[name] = {"sha": h.hexdigest(), "fit": fit, "fwd": hashlib.sha256(np.ascontiguousarray(fwd[:, mask]).tobytes()).hexdigest(),
                 "stage_evals": np.asarray(st["stage_evals"])[:, :3].tolist()}
    fb.close()
print(json.dumps(out))
'''


def _cfg():
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg["use_camera_prior"] = False
    cfg["maxiters"] = _MAXITERS
    return cfg


_RUNS = {}


def _run_jobs(**switches):
    """Both jobs in a process of their own (the lab build reads its switches once); one run per set of switches and module."""
    key = tuple(sorted(switches.items()))
    if key not in _RUNS:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(switches)
        r = subprocess.run([sys.executable, "-c", _JOB % {"root": root, "tests": os.path.join(root, "tests")}], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        _RUNS[key] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return _RUNS[key]


def _where_in_launch(stage_evals, rpb, R):
    """Every frame of a resident job runs from round 0 and consumes one evaluation per round, so its stage with index k ends in
    round (evaluations of stages 0 .. k) - 1; a polled batch of rpb rounds is launches of R rounds and a shorter last one.
    Per stage end: (frame, k, round within its launch, rounds of that launch)."""
    out = []
    for f, ev in enumerate(stage_evals):
        for k, c in enumerate(np.cumsum(ev)):
            q = (int(c) - 1) % rpb
            first = (q // R) * R
            out.append((f, k, q - first, min(R, rpb - first)))
    return out


@H.requires_lab()
@pytest.mark.parametrize("R", sorted({1, 3, 8, _R_MAX}))
def test_launch_lengths_give_the_bits_of_the_serial_loop(R):
    """17 frames, launches of R rounds in polled batches of seven (3 + 3 + 1; R = 8: one launch of seven), against the serial
    loop at that cadence: one sha256 over parameters, stage_evals, stage_loss and every row of verts, and the forward state
    left in BatchDev.fwd.  For R > 1 the job has, by its stage_evals: a frame that switches stage with rounds of the launch
    still to come (they run under the new stage, taken from the tick in LDS), and frames that finish in the first, in a middle
    and in the last round of a launch of several rounds (the finish in a round other than the first is where a workgroup saves
    the forward state that its previous export kept in LDS)."""
    ref = _run_jobs(SFX_DENSE_OVERLAP="0", SFX_POLL_ROUNDS=str(_POLL))
    out = _run_jobs(SFX_DENSE_MULTI_R=str(R), SFX_POLL_ROUNDS=str(_POLL))
    print(R, out["slices17"])
    ev = out["slices17"]["stage_evals"]
    assert min(sum(e) for e in ev) > 100, ev
    if R > 1:
        ends = _where_in_launch(ev, _POLL, R)
        last_k = len(ev[0]) - 1
        fin = [(r, n) for f, k, r, n in ends if k == last_k and n > 1]
        print("finishes (round, rounds of the launch):", sorted(set(fin)))
        assert any(r == 0 for r, n in fin), "no frame finishes in the first round of a launch"
        assert any(0 < r < n - 1 for r, n in fin), "no frame finishes in a middle round of a launch"
        assert any(r == n - 1 for r, n in fin), "no frame finishes in the last round of a launch"
        assert any(k < last_k and r < n - 1 for f, k, r, n in ends), "no frame switches stage in the middle of a launch"
    assert out == ref, (R, out, ref)      # (the pooled job too: launches of R rounds between admissions)


@H.requires_lab()
def test_admission_and_compaction_between_launches_give_the_bits_of_the_serial_loop():
    """40 frames through slots = 16 under the shipped rule against the serial loop: frames are admitted into the columns of
    finished ones between launches, so the first round of the next launch reads the state tick_admit wrote to global memory,
    not what the column's previous frame left in LDS; verts and BatchDev.fwd included."""
    ref = _run_jobs(SFX_DENSE_OVERLAP="0")
    out = _run_jobs()
    print(out["pooled40"])
    assert min(sum(e) for e in out["pooled40"]["stage_evals"]) > 100
    assert out["pooled40"] == ref["pooled40"], (out["pooled40"], ref["pooled40"])


@H.requires_lab()
def test_forward_state_in_memory_after_a_multi_round_fit():
    """BatchDev.fwd after a fit under the shipped rule (every round of these jobs in an eight-round launch) against the loop
    without the form (SFX_DENSE_MULTI=0: every export pass saves its forward state): each frame's row holds the forward
    state of its last exported evaluation -- the defined floats, see _fwd_defined -- and the fit is the same."""
    ref = _run_jobs(SFX_DENSE_MULTI="0")
    out = _run_jobs()
    for job in ("slices17", "pooled40"):
        assert out[job]["fwd"] == ref[job]["fwd"], job
        assert out[job]["fit"] == ref[job]["fit"], job


@pytest.fixture(scope="module")
def cfg_short():
    return _cfg()


@pytest.fixture(scope="module")
def batch17(synth_model, cfg_short):
    """The 17-frame job twice in this process (whichever library is loaded: the product library's shipped rule)."""
    dm = T._dm(synth_model, cfg_short)
    frames = T.synth_frames(synth_model, cfg_short, _KINDS)
    return [O._fit(dm, cfg_short, frames, _IDX17) for _ in range(2)]


def _same(a, b, rows_a, rows_b, keys=("stage_loss", "stage_evals")):
    for k in keys:
        assert np.array_equal(a[k][rows_a], b[k][rows_b]), k
    for k in a["params"]:
        assert np.array_equal(a["params"][k][rows_a], b["params"][k][rows_b]), k


def test_seventeen_frames_fitted_twice_are_byte_equal(batch17):
    a, b = batch17
    assert int(a["stage_evals"].sum()) > 17 * 100
    n = list(range(17))
    _same(a, b, n, n, keys=("loss", "grad", "stage_loss", "stage_evals", "verts"))


def test_each_of_seventeen_frames_equals_itself_alone(synth_model, cfg_short, batch17):
    """One column: every round of the frame alone is in a multi-round launch of one workgroup; in the batch its neighbours switch
    stage and finish in other rounds of the same launches."""
    dm = T._dm(synth_model, cfg_short)
    frames = T.synth_frames(synth_model, cfg_short, _KINDS)
    alone = [O._fit(dm, cfg_short, frames, [t]) for t in range(_KINDS)]
    for i, t in enumerate(_IDX17):
        _same(batch17[0], alone[t], [i], [0], keys=("loss", "grad", "stage_loss", "stage_evals"))


def test_seventeen_frames_equal_a_sub_batch_of_three(synth_model, cfg_short, batch17):
    dm = T._dm(synth_model, cfg_short)
    frames = T.synth_frames(synth_model, cfg_short, _KINDS)
    sub = O._fit(dm, cfg_short, frames, _IDX17[:3])
    _same(batch17[0], sub, [0, 1, 2], [0, 1, 2], keys=("loss", "grad", "stage_loss", "stage_evals"))
