#!/usr/bin/env python
"""bench.py -- fitted frames/s of the MI355X SMPL-X fitting engine (BASELINE.json metric).

Workload (BASELINE.json configs[1]): 256 synthetic frames per GPU, neutral SMPL-X-shaped
synthetic model, body-only (K=25 coco25), the 5-stage L-BFGS schedule of
cfg_files/fit_smplx_smplifyx.yaml with use_vposer=False + synthetic regression prior
(SURVEY.md 8d), camera stage + 5 body stages per frame.  A "step" = one complete fit of
the rank's 256 frames.  Frames are independent: rank r fits frames [r*256, (r+1)*256)
(weak scaling), no collective in the data path, one all_gather of the fitted-parameter
records at the end of every step (RCCL over xGMI when N > 1).

    python bench.py --gpus N --steps K --warmup W [--lbs dense|rows] [--frames 256] [--full] [--dump-outputs DIR]

`--gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset) starts the N ranks itself
(torch.distributed.run, one process per GPU, RCCL); under an external launcher it checks that the
launcher's world size is N.

A plain run sets up, warms up, times K steps and prints ONE JSON line on rank 0: metric, value (frames/s),
unit, higher_is_better, dtype, ms_per_step (one timed step) and the job's configuration.  `--dump-outputs DIR`
writes what the last timed step returned to DIR/<name>.npy (dump_outputs).  `--full` adds every other
measurement, and the line then carries extra objects:
  roofline          the dense LBS GEMM (k_lbs_dense16): algorithmic flops / HIP-event duration (MFMA bound)
  roofline_tick     the per-frame loss / adjoint / L-BFGS kernel (k_tick_dense): algorithmic bytes / duration
  cpu_baseline      the oracle (port of the reference path) timed on ALL host cores: latency mode
                    (1 process x all threads) and throughput mode (one single-threaded process per core)
  reference_parity  distribution of the final-loss difference to the REAL reference's fits of the golden frames
  closure_parity    the HIP closure against fp64 autograd of the oracle at seeded points
  alt, min3_camera_keypoints, configs3_single_gpu   the same job through the needed-rows path, on the
                    min-3-camera-keypoints sequence, and configs[3]'s 1 024-frame job on this GPU
  kernels_ms_avg, host   per-kernel HIP-event times of the timed steps and the host thread's side of the loop
  ranks             (N > 1) per-GPU frames/s, evaluation counts and the time of the RCCL gather
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

PEAK_MFMA_F32 = 157.3e12      # MI355X_MICROARCH.md: fp32 MFMA = fp32 vector peak
PEAK_HBM = 8.0e12


# ------------------------------------------------------------------------------------------------------------------
# The ONE line of the contract carries numbers and short tags only (< LINE_LIMIT bytes, strict JSON: the driver keeps the
# last 8 000 bytes of stdout and parses the line from there -- round 3's 20-KB line was cut and counted as unmeasured);
# everything else -- per-frame arrays, per-stage lists, the prose that explains a figure -- goes to the detail file
# (gpurun_out/bench_detail_<tag>.json, copied into profiles/ for the rounds' records) and to stderr.
LINE_LIMIT = 4096


def _num(v, sig=6):
    """JSON-safe scalar: floats rounded to `sig` significant digits, NaN / inf -> None, numpy scalars -> python."""
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    v = float(v)
    if not np.isfinite(v):
        return None
    return float("%.*g" % (sig, v))


def _pick(d, keys, sig=6):
    return {k: _num(d[k], sig) for k in keys if d is not None and k in d and not isinstance(d[k], (list, dict, tuple))}


def sanitize(o):
    """Deep copy of a report with every NaN / inf replaced by None and numpy types unwrapped (strict JSON)."""
    if isinstance(o, dict):
        return {str(k): sanitize(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [sanitize(v) for v in o]
    if isinstance(o, np.ndarray):
        return sanitize(o.tolist())
    if isinstance(o, (np.floating, float)):
        return float(o) if np.isfinite(o) else None
    if isinstance(o, np.integer):
        return int(o)
    return o


ROOFLINE_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "frac_executed", "mfma_busy_frac",
                 "avg_launch_us", "avg_launch_us_profile", "launches", "frames_per_launch", "share_of_step", "hbm_frac", "bytes_per_launch",
                 "bytes_per_frame_launch", "rows_per_frame_launch", "shared_bytes_per_launch", "l2_stream_bytes_per_frame", "l2_stream_GBps_per_cu",
                 "columns_per_launch", "bytes_per_column_launch",
                 "grid_entries_per_column", "pairs_per_column", "launches_per_round")


def compact_line(full):
    """The contract line from the full report: contract keys verbatim, every object reduced to its scalar figures."""
    line = {k: _num(full.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                           "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    cfg = full.get("config", {})
    line["config"] = _pick(cfg, ("workload", "frames_per_gpu", "lbs_mode", "gemm_columns_per_gpu", "parallelism",
                                 "closure_evals_per_frame_mean", "closure_evals_per_frame_max", "closure_evals_per_s",
                                 "reference_equiv_evals_per_frame_mean", "final_loss_mean", "final_loss_median", "non_finite",
                                 "configs3_single_gpu_frames_per_s", "single_gpu_same_job_frames_per_s", "per_gpu_frames_per_s_min", "per_gpu_frames_per_s_mean",
                                 "per_gpu_closure_evals_max", "gather_ms_max"))
    for name in ("roofline", "roofline_tick", "roofline_pen"):
        if name in full:
            line[name] = _pick(full[name], ROOFLINE_KEYS)
            line[name].setdefault("traffic", None)
    cb = full.get("cpu_baseline")
    if cb is not None:
        line["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "sample", "mode", "closure_evals_per_s", "cpu_model", "error"))
    rp = full.get("reference_parity")
    if rp is not None:      # second half of BASELINE's metric: final-loss delta vs the reference's own fits
        line["reference_parity"] = _pick(rp, ("frames", "final_loss_rel_delta_mean", "final_loss_rel_delta_median",
                                              "final_loss_rel_delta_signed_mean", "reference_f32_vs_f64_rel_delta_mean",
                                              "reference_f32_vs_f64_rel_delta_median", "camera_stage_loss_rel_delta_max",
                                              "closure_evals_mean", "reference_closure_evals_f32_mean", "error"), sig=4)
    cp = full.get("closure_parity")
    if cp is not None:
        line["closure_parity"] = _pick(cp, ("loss_rel_err_max", "grad_rel_err_max", "error"), sig=3)
    if "value_min3_camera_keypoints" in full:
        line["value_min3_camera_keypoints"] = _num(full["value_min3_camera_keypoints"])
    if isinstance(full.get("alt"), dict):
        line["alt"] = _pick(full["alt"], ("lbs_mode", "value", "unit", "ms_per_step", "closure_evals_per_frame_mean", "final_loss_median"))
    if isinstance(full.get("host"), dict):
        line["host"] = _pick(full["host"], ("enqueue_us_per_round", "loop_us_per_round", "kernels_us_per_round", "event_pair_us", "queue_dry_frac", "wait_frac", "outside_loop_ms_per_step"), sig=4)
    if "kernels_ms_avg" in full:
        line["kernels_ms_avg"] = _pick(full["kernels_ms_avg"], ("lbs_dense", "tick_dense", "fit_rows", "penetration"))
    if "detail" in full:
        line["detail"] = full["detail"]
    # strings are tags: anything longer than 160 characters is prose and belongs to the detail file
    def clip(o):
        if isinstance(o, dict):
            return {k: clip(v) for k, v in o.items()}
        return o[:160] if isinstance(o, str) else o
    line = clip(line)
    # never exceed the limit: shed the optional objects, least essential first
    for drop in ("kernels_ms_avg", "host", "alt", "closure_parity", "roofline_pen", "roofline_tick", "reference_parity"):
        if len(json.dumps(line, allow_nan=False)) < LINE_LIMIT:
            break
        line.pop(drop, None)
    return line


def write_detail(full, tag):
    """The long form of the report: gpurun_out/bench_detail_<tag>.json (merged back from the GPU box; the rounds' records
    are copied into profiles/).  Returns the path relative to the repository root, or None if it could not be written."""
    rel = os.path.join("gpurun_out", "bench_detail_%s.json" % tag)
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, rel), "w") as f:
            json.dump(sanitize(full), f, indent=1, allow_nan=False)
        return rel
    except Exception as e:          # a read-only tree must not cost the measurement
        print("[bench] detail file not written: %r" % e, file=sys.stderr)
        return None


DUMP_LIMIT = 64 << 20       # bytes: --dump-outputs writes at most this much


def dump_outputs(dirname, res, records):
    """--dump-outputs DIR: what the last timed step returned -- every array of driver.fit_frames' result (this rank's
    frames: fitted parameters, per-stage losses and evaluation counts) and the gathered records of all frames
    (`records`) -- as DIR/<name>.npy.  float32 arrays stay float32, everything else (float64, integer and boolean
    counts and flags: exact) is written as float64.  Above DUMP_LIMIT bytes in all, every array keeps the same seeded
    sample of its rows (frames), listed in DIR/<name>_rows.npy.  Returns {name: shape} of what was written."""
    arrays = dict(res)
    arrays["records"] = records
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    arrays = {k: (a if a.dtype == np.float32 else a.astype(np.float64)) for k, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    keep = 1.0
    if total > DUMP_LIMIT:      # what a sample costs per row kept: the row and its index in <name>_rows.npy (1 % left for headers)
        keep = 0.99 * DUMP_LIMIT / (total + sum(8 * a.shape[0] for a in arrays.values() if a.ndim > 0))
    os.makedirs(dirname, exist_ok=True)
    written = {}
    for k in sorted(arrays):
        a = arrays[k]
        if keep < 1.0 and a.ndim > 0 and a.shape[0] > 1:
            n = a.shape[0]
            rows = np.sort(np.random.RandomState(0).choice(n, max(1, int(n * keep)), replace=False))
            a = a[rows]
            np.save(os.path.join(dirname, k + "_rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(dirname, k + ".npy"), np.ascontiguousarray(a))
        written[k] = list(a.shape)
    return written


def item_rows_by_class(joint_map, n_extra, n_lmk, nbj):
    """Vertex items (blend-shape row triples) under the live keypoints of the three stage classes -- body only | + hands |
    all -- for a joint map (SFX model source indices: < 55 kinematic joint, then extra vertices (1 item), static landmarks
    (3 items: face corners), dynamic contour landmarks (3 items)); keypoints are ordered body | hands (42) | face.
    Returns (all items per class, of which dynamic-contour items per class)."""
    src = np.asarray(joint_map).tolist()
    per_k = [0 if s_ < 55 else (1 if s_ < 55 + n_extra else 3) for s_ in src]
    dyn_k = [3 if s_ >= 55 + n_extra + n_lmk else 0 for s_ in src]
    K = len(per_k)
    cut = [min(K, nbj), min(K, nbj + 42), K]
    return [int(sum(per_k[:c])) for c in cut], [int(sum(dyn_k[:c])) for c in cut]


def tick_bytes(rows_static, rows_dynamic, n_var_live, use_vposer, vposer_bytes=0.0, kd=506, hist=100):
    """Algorithmic HBM bytes of k_tick_dense: (shared per launch, per frame and launch).
    Shared by every frame of a launch -- read from HBM once, like the GEMM's blend-shape matrix: the adjoint's 3 blend-shape
    rows (kd floats + 16 B of skinning) per STATIC live vertex item (forward offsets come from the GEMM), and with VPoser the
    decoder's weights forward (next pose) and transposed (gradient).  Per frame: the rows of its dynamic-contour items (they
    follow the head pose), the two-loop recursion's 2 x hist history rows of the live optimiser variables, 8 work vectors.
    What one FRAME streams through its compute unit's L2 port per launch is shared + per-frame: that, not HBM, is what the
    kernel waits for (`l2_stream_*` keys)."""
    row = (3 * kd + 16) * 4.0
    shared = rows_static * row + (2.0 * vposer_bytes if use_vposer else 0.0)
    per_frame = rows_dynamic * row + 2.0 * hist * n_var_live * 4.0 + 8 * n_var_live * 4.0
    return shared, per_frame


# The headline (`value`) is measured on SURVEY.md 8(d)'s generator VERBATIM: confidences U(0.3, 1), 10 % of the keypoints
# dropped, nothing else -- the sequence rounds 1 and 2 (first half) were measured on.  About 5 % of those frames lose two
# of the four camera-initialisation keypoints; their camera is under-determined (the reference's own fp32 / fp64 runs
# land in different basins on them) and they take 2-3 x the evaluations, so ONE of them decides the time of the rank
# that draws it.  The same job on a detector that keeps at least 3 of the 4 camera-initialisation keypoints
# (round 2's headline sequence) is reported beside it as `value_min3_camera_keypoints`.
MIN_CAMERA_KEYPOINTS = 3


def build_cfg(workload="body"):
    """body: BASELINE configs[1] (body-only keypoints, use_vposer=False + synthetic regression prior).
    full: BASELINE configs[2] (hands + face + contour, K=135, VPoser decode in the loop, z0 = 0);
    pen: BASELINE configs[4] (cfg_files/fit_smplx_combined_halpe.yaml VERBATIM: hands + face, K = 136, combined regression
    prior, camera prior, interpenetration term; on synthetic.make_topology_model: the real SMPL-X topology, part table and
    ExPose body of the reference tree -- `--mesh tubes`: the surface-like synthetic mesh of rounds 2-4) --
    side measurements (`--workload full|pen`), never the headline."""
    from smplifyx_amd import cmd_parser
    over = dict(interpenetration=False, visualize=False, interactive=False, save_vertices=False,
                use_gender_classifier=False)
    if workload == "body":
        over.update(use_hands=False, use_face=False, use_vposer=False)
    if workload == "pen":
        # the cfg verbatim: hands + face + contour (halpe K = 136), regression prior 'combined', camera prior,
        # use_conf_for_camera_init, interpenetration (max_collisions 128, df_cone_height 1e-4, coll_loss_weights [0, 0.1, 1])
        cfg = cmd_parser.load_config(os.path.join(ROOT, "cfg_files", "fit_smplx_combined_halpe.yaml"),
                                     dict(visualize=False, interactive=False, save_vertices=False, use_gender_classifier=False))
        assert cfg["interpenetration"] and cfg["use_hands"] and cfg["use_face"] and cfg["use_camera_prior"]
        return cfg
    cfg = cmd_parser.load_config(os.path.join(ROOT, "cfg_files", "fit_smplx_smplifyx.yaml"), over)
    cfg["use_camera_prior"] = False
    return cfg


def lbs_flops_per_frame(V, KD=506, J=55):
    return 2.0 * KD * 3 * V + 2.0 * J * 12 * V + 21.0 * V


def lbs_flops_executed_per_frame(V, mean_tile_joints, KDP=512):
    """MFMA flops the kernel actually issues: K padded to 512; the skinning GEMM only visits the
    joints that carry weight in each 16-vertex tile (structural zeros of lbs_weights skipped)."""
    return 2.0 * KDP * 3 * V + 2.0 * mean_tile_joints * 12 * V + 21.0 * V


def lbs_bytes_per_launch(B, V, KD=506, J=55):
    const = 4.0 * (KD * 3 * V + J * V + 3 * V)              # dirs + W + template
    return const + B * (3.0 * V * 4 + (KD + 12 * J) * 4)    # vertices out + feat/A in


def _cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _usable_cores():
    """Cores this process may actually use: affinity mask and cgroup CPU quota (a container on a 256-thread host may own
    a few of them), next to os.cpu_count()."""
    n = os.cpu_count() or 1
    info = {"os_cpu_count": n}
    try:
        a = len(os.sched_getaffinity(0)); info["affinity"] = a; n = min(n, a)
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            q, per = open(path).read().split()[:2]
            info["cgroup_cpu_max"] = "%s %s" % (q, per)
            if q != "max":
                n = min(n, max(1, int(float(q) / float(per))))
        except Exception:
            pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        info["cgroup_v1_quota"] = "%d %d" % (q, per)
        if q > 0:
            n = min(n, max(1, q // per))
    except Exception:
        pass
    info["usable"] = n
    return n, info


def _cpu_worker(task):
    """One oracle frame fit for `budget` seconds with `threads` torch threads; returns closure evaluations
    and the seconds they took.  Runs in a forked child (before this process touches the GPU)."""
    frame, threads, budget = task
    import helpers as H
    torch.set_num_threads(threads)
    st = _CPU_STATE
    ff = H.oracle_frame_fit(st["model"], st["cfg"], st["frames"], frame % st["n"], dtype=torch.float32)

    class _Stop(Exception):
        pass
    t0 = time.time()
    n = [0]
    orig = ff._make_closure

    def mk(params, fn):
        closure, groups = orig(params, fn)

        def timed(x):
            if time.time() - t0 > budget:
                raise _Stop()
            n[0] += 1
            return closure(x)
        return timed, groups
    ff._make_closure = mk
    try:
        ff.run()
    except _Stop:
        pass
    return n[0], time.time() - t0


_CPU_STATE = {}


def cpu_baseline_measure(budget_latency=10.0, budget_throughput=14.0):
    """the oracle (port of the reference's path, validated against the reference by
    tests/golden) on the node's own host cores, (i) latency mode: 1 process x torch.set_num_threads(all
    cores), (ii) throughput mode: one single-threaded process per core over disjoint frames.  Called BEFORE the
    GPU is initialised (the workers are forked).  Returns closure evaluations per second for both modes."""
    import multiprocessing as mp
    import helpers as H
    from smplifyx_amd import synthetic
    torch.set_num_threads(1)        # no thread pool in the parent before the fork
    cores, core_info = _usable_cores()
    print("[bench] host cores: %s" % core_info, file=sys.stderr)
    cfg = build_cfg("body")
    model = synthetic.make_synthetic_model(0)
    K = len(H.joint_map_for(cfg))
    nproc = min(cores, int(os.environ.get("SFX_CPU_BASELINE_MAX_PROCS", "128")))
    nfr = min(nproc, 16)
    frames = synthetic.make_frames(nfr, H.oracle_joints_fn(model, cfg), K, focal=float(cfg.get("focal_length") or 5000.0))
    _CPU_STATE.update(model=model, cfg=cfg, frames=frames, n=nfr)
    ctx = mp.get_context("fork")
    with ctx.Pool(1) as pool:
        n1, t1 = pool.map(_cpu_worker, [(0, cores, budget_latency)])[0]
    with ctx.Pool(nproc) as pool:
        res = pool.map(_cpu_worker, [(i, 1, budget_throughput) for i in range(nproc)], chunksize=1)
    _CPU_STATE.clear()
    print("[bench] cpu baseline: latency %d evals in %.1f s (%d threads); throughput %s" % (
        n1, t1, cores, [(n, round(t, 1)) for n, t in res][:16]), file=sys.stderr)
    return {"cores": cores, "core_info": core_info, "cpu_model": _cpu_model_name(),
            "latency_evals_per_s": n1 / t1, "latency_threads": cores, "latency_evals": n1, "latency_s": t1,
            "throughput_evals_per_s": float(sum(n / t for n, t in res)), "throughput_processes": nproc,
            "throughput_evals": int(sum(n for n, _ in res)), "throughput_s": float(max(t for _, t in res))}


def cpu_baseline_report(m, ref_evals_per_frame):
    """evaluations/s -> frames/s with the reference-equivalent evaluations one fitted frame takes (measured on the GPU
    run of the same workload); `value` is the better of the two modes (the throughput mode on any multi-core host)."""
    per = max(ref_evals_per_frame, 1.0)
    lat, thr = m["latency_evals_per_s"] / per, m["throughput_evals_per_s"] / per
    return {"value": max(lat, thr), "unit": "frames/s", "cores": m["cores"], "kind": "port", "cpu_model": m["cpu_model"],
            "host": m["core_info"],
            "mode": "throughput" if thr >= lat else "latency",
            "latency": {"value": lat, "processes": 1, "threads": m["latency_threads"], "closure_evals_per_s": m["latency_evals_per_s"]},
            "throughput": {"value": thr, "processes": m["throughput_processes"], "threads_per_process": 1,
                           "closure_evals_per_s": m["throughput_evals_per_s"]},
            "closure_evals_per_s": max(m["latency_evals_per_s"], m["throughput_evals_per_s"]),
            "sample": "EXTRAPOLATED from evals/s: oracle fit (torch fp32) of this job's frames 0..%d: %d procs x 1 thread x %.0f s = %d closure evals; / %.0f evals per fitted frame" % (
                m["throughput_processes"] - 1, m["throughput_processes"], m["throughput_s"], m["throughput_evals"], per),
            "sample_detail": {"latency_mode": "1 process x %d threads on frame 0 for %.0f s = %d evaluations" % (m["latency_threads"], m["latency_s"], m["latency_evals"]),
                              "throughput_mode": "%d single-threaded processes on frames 0..%d for %.0f s = %d evaluations" % (
                                  m["throughput_processes"], m["throughput_processes"] - 1, m["throughput_s"], m["throughput_evals"]),
                              "closure": "dense LBS forward + autograd backward per evaluation",
                              "evals_per_fitted_frame": per}}


def event_pair_overhead_us(n=200):
    """Median elapsed time of a HIP-event pair with nothing between them on the current stream (microseconds)."""
    import torch
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)


def csrc_sha():
    """Hash of the kernel sources this build was made from (same function as tools/pmc_summary.py)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "smplify-x-partial_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")) and f != "api.hip":      # (api.hip is the host layer: loops, launches, allocation -- not what the counters measure)
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_is_current(path):
    """Counter traffic is REPLAYED from profiles/pmc_summary.json (counters cannot be read inside an un-profiled run);
    it is only valid for the kernels it was taken with: the summary carries the hash of csrc/ at profiling time."""
    name = "profiles/" + os.path.basename(path)
    if not os.path.exists(path):
        return False, "no " + name
    try:
        sha = json.load(open(path)).get("_meta", {}).get("csrc_sha")
    except Exception as e:
        return False, "unreadable pmc summary: %r" % e
    if sha is None:
        return False, name + " carries no csrc hash (taken before round 3): traffic not replayed"
    cur = csrc_sha()
    if sha != cur:
        return False, name + " was taken with csrc %s, this build is %s: traffic not replayed (stale)" % (sha, cur)
    return True, None


def self_consistent_frames(r32_stages, r64_stages, limit=0.25):
    """Frames on which the reference agrees with ITSELF: its fp32 and fp64 runs stay within `limit` (relative) of each
    other after every stage.  A frame that fails this (benchmark frame 51: 401 vs 2 730 after the fourth body stage, two
    of its four camera-init keypoints missing) has more than one basin; which one a run ends in is not a property of
    the arithmetic being tested, so such frames are listed, not averaged."""
    r32_stages, r64_stages = np.asarray(r32_stages, np.float64), np.asarray(r64_stages, np.float64)
    return (np.abs(r64_stages - r32_stages) / np.abs(r32_stages)).max(1) <= limit


def parity_stats(ours, r32, r64, scored=None):
    """Distribution of the final-loss difference to the reference's fp32 fits, with the reference's own fp64-vs-fp32
    difference over the same frames as the yardstick (the optimisation is chaotic: single frames differ by per cent
    between any two correctly rounded runs, the DISTRIBUTIONS have to agree).  `scored`: boolean mask of the frames
    that enter the statistics (self_consistent_frames); the others are reported one by one."""
    ours, r32, r64 = (np.asarray(a, np.float64) for a in (ours, r32, r64))
    listed = None
    if scored is not None:
        scored = np.asarray(scored, bool)
        listed = [{"frame": int(i), "final_loss": float(ours[i]), "reference_f32": float(r32[i]), "reference_f64": float(r64[i])}
                  for i in np.flatnonzero(~scored)]
        ours, r32, r64 = ours[scored], r32[scored], r64[scored]
    d = (ours - r32) / r32                      # signed relative difference per frame
    y = (r64 - r32) / r32                       # the reference against itself
    n_low = int((ours < r32).sum())
    out = {"frames": int(ours.size),
           "final_loss_rel_delta_mean": float(np.mean(np.abs(d))), "final_loss_rel_delta_median": float(np.median(np.abs(d))),
           "final_loss_rel_delta_signed_mean": float(np.mean(d)), "final_loss_rel_delta_signed_median": float(np.median(d)),
           "reference_f32_vs_f64_rel_delta_mean": float(np.mean(np.abs(y))), "reference_f32_vs_f64_rel_delta_median": float(np.median(np.abs(y))),
           "reference_f64_minus_f32_signed_mean": float(np.mean(y)), "reference_f64_minus_f32_signed_median": float(np.median(y)),
           "frames_below_reference_f32": n_low, "frames_above_reference_f32": int((ours > r32).sum()),
           "reference_f64_below_f32_frames": int((r64 < r32).sum()),
           # quantiles of |difference|: ours against the reference's fp32 run, next to the reference's fp64 against its fp32
           "final_loss_rel_delta_p90": float(np.percentile(np.abs(d), 90)), "final_loss_rel_delta_max": float(np.abs(d).max()),
           "reference_f32_vs_f64_rel_delta_p90": float(np.percentile(np.abs(y), 90)),
           "reference_f32_vs_f64_rel_delta_max": float(np.abs(y).max()),
           "mean_final_loss": float(ours.mean()), "reference_mean_final_loss_f32": float(r32.mean()),
           "reference_mean_final_loss_f64": float(r64.mean()),
           "median_final_loss": float(np.median(ours)), "reference_median_final_loss_f32": float(np.median(r32)),
           "reference_median_final_loss_f64": float(np.median(r64))}
    if listed is not None:
        out["frames_not_scored"] = listed
        out["frames_not_scored_reason"] = ("the reference's own fp32 and fp64 runs differ by more than 25 % after some stage "
                                           "on these frames (several basins): listed, not averaged")
    try:
        from scipy.stats import binomtest, wilcoxon
        out["paired_sign_test_p_vs_reference_f32"] = float(binomtest(n_low, int((ours != r32).sum()), 0.5).pvalue)
        out["paired_wilcoxon_p_vs_reference_f32"] = float(wilcoxon(ours, r32).pvalue)
        out["reference_f64_vs_f32_paired_wilcoxon_p"] = float(wilcoxon(r64, r32).pvalue)
    except Exception:
        pass
    return out


def load_bench_golden(raw):
    """tests/golden/e2e_bench.npz holds the reference's fits of frames 0-63 of the min-3-camera-keypoints sequence;
    the raw 8(d) sequence differs from it in two frames (23, 51: two camera keypoints dropped), whose raw keypoints and
    reference fits are kept in e2e_bench_raw_delta.npz (tools/make_goldens.py e2e_bench_raw_delta)."""
    path = os.path.join(ROOT, "tests", "golden", "e2e_bench.npz")
    if not os.path.exists(path):
        return None
    g = dict(np.load(path))
    if raw:
        dpath = os.path.join(ROOT, "tests", "golden", "e2e_bench_raw_delta.npz")
        if not os.path.exists(dpath):
            return None
        d = np.load(dpath)
        for q, i in enumerate(d["frames"]):
            for k in ("keypoints", "reg_pose", "reg_global"):
                g[k] = g[k].copy(); g[k][i] = d[k][q]
            for k in d.files:
                if k.startswith("f%d_" % i):
                    g[k] = d[k]
    return g


def reference_parity(model, lbs_mode, raw=True):
    """Second half of BASELINE's metric ("mean reprojection-loss delta vs reference"): the first N frames of this
    benchmark's synthetic sequence were fitted by the REAL reference with this benchmark's configuration
    (smplifyx/fit_single_frame.py imported in the build container, fp32 and fp64; tools/make_goldens.py
    e2e_bench -> tests/golden/e2e_bench.npz); fit the same frames here and report the distribution of the
    final-loss difference next to the reference's own fp32-vs-fp64 difference."""
    from smplifyx_amd import driver, engine, utils as U
    g = load_bench_golden(raw)
    if g is None:
        return None
    cfg = build_cfg("body")
    jm = U.smpl_to_annotation("smplx", use_hands=False, use_face=False, use_face_contour=cfg["use_face_contour"],
                              format=cfg["format"])
    dm = engine.DeviceModel(model, joint_map=jm, num_betas=cfg["num_betas"],
                            num_expression_coeffs=cfg["num_expression_coeffs"], num_pca_comps=cfg["num_pca_comps"],
                            use_face_contour=cfg["use_face_contour"])
    jw = np.ones(len(jm), np.float32)
    ign = cfg.get("joints_to_ign")
    if ign is not None and -1 not in ign:
        jw[ign] = 0.0
    n = g["keypoints"].shape[0]
    res = driver.fit_frames(dm, cfg, g["keypoints"], jw, 600, 800, 5000.0, reg_pose=g["reg_pose"],
                            reg_global=g["reg_global"], lbs_mode=lbs_mode, reuse_entry_eval=True)
    ours = res["stage_loss"]                                              # [n, 1 + stages]
    r32 = np.stack([g["f%d_f32_losses" % i] for i in range(n)])
    r64 = np.stack([g["f%d_f64_losses" % i] for i in range(n)])
    ok = self_consistent_frames(r32, r64)
    out = parity_stats(ours[:, -1], r32[:, -1], r64[:, -1], scored=ok)
    ours_all, r32_all, r64_all = ours, r32, r64
    ours, r32, r64 = ours[ok], r32[ok], r64[ok]
    out.update({
        "source": "tests/golden/e2e_bench%s.npz: reference fit_single_frame (fp32 / fp64) on frames 0-%d of the %s "
                  "sequence, this benchmark's configuration" % ("+e2e_bench_raw_delta" if raw else "", n - 1,
                                                                "SURVEY 8(d) (headline)" if raw else "min-3-camera-keypoints"),
        "lbs_mode": lbs_mode,
        "camera_stage_loss_rel_delta_max": float(np.max(np.abs(ours[:, 0] - r32[:, 0]) / np.abs(r32[:, 0]))),
        "per_stage_loss_rel_delta_mean": [float(np.mean(np.abs(ours[:, k] - r32[:, k]) / np.abs(r32[:, k]))) for k in range(ours.shape[1])],
        "per_stage_loss_rel_delta_signed_mean": [float(np.mean((ours[:, k] - r32[:, k]) / np.abs(r32[:, k]))) for k in range(ours.shape[1])],
        "reference_f32_vs_f64_per_stage_rel_delta_mean": [float(np.mean(np.abs(r64[:, k] - r32[:, k]) / np.abs(r32[:, k]))) for k in range(ours.shape[1])],
        "reference_f64_minus_f32_per_stage_signed_mean": [float(np.mean((r64[:, k] - r32[:, k]) / np.abs(r32[:, k]))) for k in range(ours.shape[1])],
        "closure_evals_mean": float(res["stage_evals"].sum(1).mean()),
        "reference_equiv_evals_mean": float(res["stage_ref_evals"].sum(1).mean()),
        "reference_closure_evals_f32_mean": float(np.mean([g["f%d_f32_evals" % i].sum() for i in range(n)])),
        "reference_closure_evals_f64_mean": float(np.mean([g["f%d_f64_evals" % i].sum() for i in range(n)])),
        "frames_fitted": int(n),
        "final_loss": [float(x) for x in ours_all[:, -1]],
        "reference_final_loss_f32": [float(x) for x in r32_all[:, -1]], "reference_final_loss_f64": [float(x) for x in r64_all[:, -1]],
        "note": "per stage: camera stage, then the 5 body stages.  signed = (ours - reference fp32) / reference fp32; the "
                "reference's fp64 run against its fp32 run over the same frames is the yardstick.  The keypoint forward of "
                "this engine (rotations, kinematic chain, keypoint-vertex skinning, projection) is carried in fp64, so its "
                "gradient noise is below torch fp32's: it is expected between the reference's fp32 and fp64 results"})
    return out


def load_pen_golden():
    """tests/golden/e2e_pen_set.npz (tools/make_goldens.py e2e_pen_set): the REAL reference's fits of frames of the `--workload pen`
    job WITH the interpenetration term -- fitting.py:437-455 as it stands, over CPU stand-ins for the three objects of the absent
    mesh_intersection package (oracle/mesh_intersection_cpu.py) -- fp32 and fp64, and fp32 without the term.  Returns a dict of
    stacked arrays in the golden's frame order, or None when the file is absent."""
    path = os.path.join(ROOT, "tests", "golden", "e2e_pen_set.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    fr = [int(i) for i in g["frames"]]
    st = lambda fmt: np.stack([g[fmt % i] for i in fr])
    out = dict(frames=np.array(fr), keypoints=st("f%d_keypoints"), reg_pose=st("f%d_reg_pose"), reg_global=st("f%d_reg_global"),
               cam_prior_t=st("f%d_cam_prior_t"), r32=st("f%d_f32_losses"), r64=st("f%d_f64_losses"), r32_noterm=st("f%d_f32_noterm_losses"),
               e32=np.array([g["f%d_f32_evals_all" % i].sum() for i in fr]), e64=np.array([g["f%d_f64_evals_all" % i].sum() for i in fr]),
               e32_noterm=np.array([g["f%d_f32_noterm_evals_all" % i].sum() for i in fr]),
               n_orient=np.array([2 if len(g["f%d_f32_losses_all" % i]) == 7 else 1 for i in fr]),
               kept32=st("f%d_f32_kept_orientation"), kept64=st("f%d_f64_kept_orientation"),
               finite32=st("f%d_f32_finite"), finite64=st("f%d_f64_finite"),
               cut32=st("f%d_f32_bvh_pairs_cut"), cut64=st("f%d_f64_bvh_pairs_cut"),
               maxpairs32=st("f%d_f32_bvh_max_pairs"), maxpairs64=st("f%d_f64_bvh_max_pairs"))
    return out


def fit_pen_golden(dm, cfg, g, lbs_mode="dense", interpenetration=True):
    """The golden frames of load_pen_golden() through driver.fit_frames the way `--workload pen` fits its frames."""
    from smplifyx_amd import driver
    n, K = g["keypoints"].shape[:2]
    jw = np.ones(K, np.float32)
    ign = cfg.get("joints_to_ign")
    if ign is not None and -1 not in ign:
        jw[ign] = 0.0
    c = dict(cfg); c["interpenetration"] = bool(interpenetration)
    return driver.fit_frames(dm, c, g["keypoints"], jw, 600, 800, 5000.0, reg_pose=g["reg_pose"], reg_global=g["reg_global"],
                             cam_prior_t=g["cam_prior_t"], cam_prior_center=np.tile(np.array([400.0, 300.0], np.float32), (n, 1)),
                             lbs_mode=lbs_mode, reuse_entry_eval=True)


def reference_parity_pen(dm, cfg, lbs_mode):
    """configs[4]'s half of "mean reprojection-loss delta vs reference": the golden frames of tests/golden/e2e_pen_set.npz fitted
    here with the term, per stage against the reference's fp32 fits, the reference's own fp64-vs-fp32 difference beside it; the
    frames on which the reference's BVH stand-in met a folded mesh (cap of max_collisions partners binding) are named."""
    g = load_pen_golden()
    if g is None:
        return None
    res = fit_pen_golden(dm, cfg, g, lbs_mode)
    ours, r32, r64 = res["stage_loss"].astype(np.float64), g["r32"], g["r64"]
    fin = np.isfinite(ours).all(1) & np.isfinite(r32).all(1) & np.isfinite(r64).all(1)
    out = parity_stats(ours[fin, -1], r32[fin, -1], r64[fin, -1])
    rel = lambda a, b: (a - b) / np.abs(b)
    out.update({
        "source": "tests/golden/e2e_pen_set.npz: the reference's fit_single_frame WITH the interpenetration term (fitting.py:437-455 over "
                  "CPU stand-ins for mesh_intersection built on oracle/penetration.py), fp32 / fp64, frames %s of the --workload pen sequence"
                  % g["frames"].tolist(),
        "lbs_mode": lbs_mode, "frames_fitted": int(len(fin)), "frames_scored": int(fin.sum()),
        "non_finite_here": g["frames"][~np.isfinite(ours).all(1)].tolist(),
        "non_finite_reference_f32": g["frames"][~np.isfinite(r32).all(1) | ~g["finite32"].astype(bool)].tolist(),
        "non_finite_reference_f64": g["frames"][~np.isfinite(r64).all(1) | ~g["finite64"].astype(bool)].tolist(),
        "camera_stage_loss_rel_delta_max": float(np.max(np.abs(rel(ours[fin, 0], r32[fin, 0])))),
        "per_stage_loss_rel_delta_mean": [float(np.mean(np.abs(rel(ours[fin, k], r32[fin, k])))) for k in range(ours.shape[1])],
        "per_stage_loss_rel_delta_median": [float(np.median(np.abs(rel(ours[fin, k], r32[fin, k])))) for k in range(ours.shape[1])],
        "per_stage_loss_rel_delta_signed_median": [float(np.median(rel(ours[fin, k], r32[fin, k]))) for k in range(ours.shape[1])],
        "reference_f32_vs_f64_per_stage_rel_delta_mean": [float(np.mean(np.abs(rel(r64[fin, k], r32[fin, k])))) for k in range(ours.shape[1])],
        "reference_f32_vs_f64_per_stage_rel_delta_median": [float(np.median(np.abs(rel(r64[fin, k], r32[fin, k])))) for k in range(ours.shape[1])],
        "closure_evals_mean": float(res["stage_evals"].sum(1).mean()),
        "reference_closure_evals_f32_mean": float(g["e32"].mean()), "reference_closure_evals_f64_mean": float(g["e64"].mean()),
        "reference_frames_with_a_folded_mesh_f32": g["frames"][g["cut32"] > 0].tolist(),
        "reference_frames_with_a_folded_mesh_f64": g["frames"][g["cut64"] > 0].tolist(),
        "frames_flagged_order_dependent_here": g["frames"][np.asarray(res.get("pen_order_dependent", np.zeros(len(fin), bool)), bool)].tolist(),
        "final_loss": [float(x) for x in ours[:, -1]],
        "reference_final_loss_f32": [float(x) for x in r32[:, -1]], "reference_final_loss_f64": [float(x) for x in r64[:, -1]],
        "note": "per stage: camera stage, then the 3 body stages of fit_smplx_combined_halpe.yaml (collision weights 0, 0.1, 1).  A "
                "'folded mesh' = an evaluation in which some triangle met more than max_collisions = 128 partners (a trial step of the "
                "line search pushed limbs through each other): the reference path reaches such states as well (DESIGN.md)"})
    return out


def closure_parity(model, workload, lbs_mode):
    """Closure-level parity of THIS build, measured in this run: the HIP closure (C ABI) against fp64 autograd of the
    oracle (checker only) at seeded points of 3 synthetic frames, camera stage and every body stage: observed maximum
    relative error of the loss and of the gradient (2-norm), next to the bounds the GPU test-suite asserts
    (tests/helpers.py: loss 1e-5 = SURVEY 8d, gradient 1e-4 = north_star)."""
    import helpers as H
    import test_gpu_parity as T
    from smplifyx_amd import synthetic
    if workload == "body":
        cfg = H.load_cfg("fit_smplx_smplifyx.yaml", use_hands=False, use_face=False, use_vposer=False); vp = None
    elif workload == "full":
        cfg = H.load_cfg("fit_smplx_smplifyx.yaml"); vp = synthetic.make_synthetic_vposer(0)
    else:
        cfg = H.load_cfg("fit_smplx_combined_halpe.yaml"); vp = None       # (keypoint terms; the interpenetration term has its own tests)
    cfg["use_camera_prior"] = False
    res = T.closure_probe(model, cfg, lbs_mode, "bench-%s-%s" % (workload, lbs_mode), vposer=vp, check=False)
    stages = sorted(res)
    return {"against": "fp64 autograd of the oracle (port of the reference objective)", "lbs_mode": lbs_mode, "frames": 3,
            "stages": stages, "loss_rel_err_max_per_stage": [res[k][0] for k in stages],
            "grad_rel_err_max_per_stage": [res[k][1] for k in stages],
            "loss_rel_err_max": max(res[k][0] for k in stages), "grad_rel_err_max": max(res[k][1] for k in stages),
            "bounds_asserted_by_the_gpu_tests": {"loss": H.CLOSURE_LOSS_TOL, "grad": H.CLOSURE_GRAD_TOL}}


def loss_distribution(fl):
    """Summary of a heavy-tailed set of per-frame final losses (a mean alone hides the tail)."""
    fl = np.asarray(fl, np.float64)
    ok = np.isfinite(fl)
    med = float(np.median(fl[ok])) if ok.any() else float("nan")
    return {"final_loss_mean": float(fl[ok].mean()) if ok.any() else None, "final_loss_median": med,
            "final_loss_p90": float(np.percentile(fl[ok], 90)) if ok.any() else None,
            "final_loss_max": float(fl[ok].max()) if ok.any() else None,
            "outliers_gt_3x_median": int((fl[ok] > 3.0 * med).sum()), "non_finite": int((~ok).sum())}


def paired_stats(a, b, name_a, name_b):
    """Per-frame paired comparison of two runs over the SAME frames."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)          # (a stage that ends inside its first step returns None in the reference, NaN here)
    n_bad = int((~ok).sum())
    a, b = a[ok], b[ok]
    d = (a - b) / np.maximum(np.abs(b), 1e-30)
    out = {"frames": int(a.size), "frames_without_a_finite_pair": n_bad, "signed_rel_delta_mean": float(d.mean()), "signed_rel_delta_median": float(np.median(d)),
           "abs_rel_delta_median": float(np.median(np.abs(d))), "frames_%s_lower" % name_a: int((a < b).sum()),
           "frames_%s_lower" % name_b: int((b < a).sum()), "frames_beyond_10_percent": int((np.abs(d) > 0.1).sum())}
    try:
        from scipy.stats import wilcoxon
        out["paired_wilcoxon_p"] = float(wilcoxon(a, b).pvalue)
    except Exception:
        pass
    return out


def _self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per GPU) under
    torch.distributed.run and hand its exit code back; rank 0 of the children prints the JSON line."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC (RCCL across processes on this driver)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=0, help="frames per GPU (default: 256 on one GPU = BASELINE configs[1]; 1024 "
                    "when --gpus N > 1 = configs[3], 8192 frames over 8 GPUs, SURVEY 8d)")
    ap.add_argument("--lbs", default="dense", choices=["dense", "rows"])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--workload", default="body", choices=["body", "full", "pen"])
    ap.add_argument("--prof-every", type=int, default=8, help="HIP-event-time every N-th launch of each kernel")
    ap.add_argument("--no-alt", action="store_true", help="skip the extra needed-rows measurement")
    ap.add_argument("--no-side", action="store_true", help="skip the side measurement on the min-3-camera-keypoints sequence")
    ap.add_argument("--no-parity", action="store_true", help="skip the fit of the reference's golden frames (profiling passes: "
                    "keeps their launches out of the per-kernel averages)")
    ap.add_argument("--mesh", choices=("topology", "tubes"), default="topology",
                    help="--workload pen: the real SMPL-X topology + part table + ExPose body (default), or the synthetic tubes")
    ap.add_argument("--no-configs3", action="store_true", help="N = 1: skip the extra 1 024-frame fit (configs[3]'s per-GPU job) behind the "
                    "headline")
    ap.add_argument("--slots", type=int, default=-1, help="dense mode: GEMM columns per GPU when --frames is larger (continuous "
                    "batching: retired columns are refilled from the frame queue, longest predicted fits first); 0 = one column per frame; "
                    "-1 (default) = driver.auto_slots: resident up to 512 frames, a 512-column pool beyond")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline as well (the --no-* switches above "
                    "pick from it): CPU baseline, needed-rows and min-3-camera-keypoints measurements, configs[3]'s 1 024-frame "
                    "job, reference and closure parity, per-kernel HIP-event times of the timed steps, roofline and host "
                    "figures, the detail file.  Without it the run sets up, warms up, times --steps fits and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned to DIR/<name>.npy "
                    "(float32 / float64, at most 64 MB: dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        args.no_cpu = args.no_alt = args.no_side = args.no_parity = args.no_configs3 = True
    if args.frames <= 0:
        args.frames = 256 if args.gpus == 1 else 1024

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_self_launch(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE); they must agree" % (args.gpus, world))
    # SFX_BENCH_REHEARSAL=1: every rank on GPU 0 with the gloo backend -- lets a 1-GPU box walk the
    # N > 1 control flow (barriers, max-over-ranks timing, record gather); never a measurement
    rehearsal = os.environ.get("SFX_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    full = args.workload == "full"
    pen = args.workload == "pen"
    if full or pen:
        args.no_cpu = True
    if pen:
        args.no_alt = True          # the term reads the whole mesh: the dense path is the only one
    # the CPU baseline forks its workers: measure it before this process creates a HIP context
    cpu_meas = None
    if not args.no_cpu and world == 1:
        try:
            cpu_meas = cpu_baseline_measure()
        except Exception as e:          # the baseline is a report, never the product path
            cpu_meas = {"error": repr(e)}
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or os.environ.get("SFX_FORCE_COLLECTIVE") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))

    from smplifyx_amd import engine, synthetic, utils as U
    cfg = build_cfg(args.workload)
    # --workload pen: the SMPL-X topology, part table and ExPose body the reference tree ships (tests/golden/smplx_topology.npz,
    # synthetic.make_topology_model) -- the mesh fitting.py:437-455 evaluates; --mesh tubes = rounds 2-4's surface-like stand-in
    topo = pen and args.mesh == "topology"
    if topo and not synthetic.topology_available():
        # the fixture is a local build product (tools/make_topology.py; SMPL-X licence: not committed): say so, use the tubes
        if rank == 0:
            print("bench: tests/golden/smplx_topology.npz is not there (python tools/make_topology.py builds it from the "
                  "reference tree) -- falling back to --mesh tubes", file=sys.stderr, flush=True)
        topo = False
        args.mesh = "tubes"
    model = synthetic.make_topology_model(0) if topo else synthetic.make_synthetic_model(0, surface=pen)
    jm = U.smpl_to_annotation("smplx", use_hands=cfg["use_hands"], use_face=cfg["use_face"],
                              use_face_contour=cfg["use_face_contour"], format=cfg["format"])
    dm = engine.DeviceModel(model, joint_map=jm, num_betas=cfg["num_betas"],
                            num_expression_coeffs=cfg["num_expression_coeffs"],
                            num_pca_comps=cfg["num_pca_comps"], use_face_contour=cfg["use_face_contour"],
                            vposer=synthetic.make_synthetic_vposer(0) if full else None)
    if pen:
        parts = synthetic.topology_parts() if topo else synthetic.make_synthetic_parts(model)
        dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    B = args.frames
    dev = torch.device("cuda", local_rank)

    def joints_fn(P):
        nB = P["global_orient"].shape[0]
        z = lambda n: torch.zeros([nB, n], device=dev)
        t = lambda a: torch.tensor(a, device=dev)
        _, j, _ = dm.lbs_forward(t(P["global_orient"]), t(P["body_pose"]), t(P["betas"]), z(10), z(3), z(3), z(3),
                                 z(12), z(12), return_verts=False, return_full_pose=False)
        return j.cpu().numpy()
    focal = float(cfg.get("focal_length") or 5000.0)
    frames = synthetic.make_frames(B, joints_fn, len(jm), start=rank * B, focal=focal)          # SURVEY 8(d) verbatim: the headline
    frames_min3 = None if args.no_side else synthetic.make_frames(
        B, joints_fn, len(jm), start=rank * B, focal=focal, min_camera_keypoints=MIN_CAMERA_KEYPOINTS,
        camera_keypoints=cfg.get("init_joints_idxs", (9, 12, 2, 5)))

    from smplifyx_amd import driver, dist as sdist
    if args.slots < 0:
        args.slots = driver.auto_slots(B) if args.lbs == "dense" else 0
    jw = np.ones(len(jm), np.float32)
    jw[cfg["joints_to_ign"]] = 0.0                 # COCO25.get_joint_weights (data_parser.py:159-171)
    n_total = world * B
    gather_ms = [0.0]

    cam_t_prior = cam_c_prior = None
    if pen:     # synthetic "ExPose" camera (fit_single_frame.py:359-401): the true translation + 5 cm noise, image centre
        rngc = np.random.RandomState(1000 + rank)
        cam_t_prior = (frames["cam_t"] + 0.05 * rngc.normal(size=frames["cam_t"].shape)).astype(np.float32)
        cam_c_prior = np.tile(np.array([frames["W"] * 0.5, frames["H"] * 0.5], np.float32), (B, 1))

    def one_fit(lbs_mode=None, fr=None):
        fr = frames if fr is None else fr
        res = driver.fit_frames(dm, cfg, fr["keypoints"], jw, fr["H"], fr["W"], fr["focal"],
                                reg_pose=None if full else fr["reg_pose"],
                                reg_global=None if full else fr["reg_global"],
                                cam_prior_t=cam_t_prior, cam_prior_center=cam_c_prior,
                                lbs_mode=lbs_mode or args.lbs, reuse_entry_eval=True,
                                slots=args.slots if (lbs_mode or args.lbs) == "dense" else 0)
        tg = time.time()
        rec = sdist.pack_records(res, rank * B)
        table = sdist.gather_records(rec, n_total, device=dev)      # the one collective (RCCL all_gather)
        gather_ms[0] = 1e3 * (time.time() - tg)
        assert table.shape[0] == n_total
        return res, table

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    def all_max(x):
        if dist is None:
            return x
        tt = torch.tensor([x], device=None if rehearsal else dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    for _ in range(args.warmup):
        one_fit()
    # (the persistent needed-rows kernel is launched a few dozen times per step: every launch is timed; the dense loop's
    #  thousands of launches are sampled)
    # (--full only: a plain run times the fits without HIP events between their launches)
    prof_every = 1 if args.lbs == "rows" else args.prof_every
    if args.full:
        engine.prof_enable(True, every=prof_every)
        engine.prof_reset()
        engine.loop_host_stats(reset=True)
        if pen:
            engine.pen_work_reset()
    sync()
    t0 = time.time()
    for _ in range(args.steps):
        st, table = one_fit()
    torch.cuda.synchronize()
    dt_rank = time.time() - t0                     # this rank's own time (before waiting for the others)
    sync()
    dt = all_max(time.time() - t0)
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, st, table)
        print("[bench] outputs of the last timed step in %s: %s" % (args.dump_outputs, dumped), file=sys.stderr)
    if args.full:
        engine.prof_enable(False)
        # per-kernel HIP-event figures of the headline region (read before the side runs add their launches)
        prof = {k: engine.prof_get(k) for k in ("lbs_dense", "tick", "fit_rows", "penetration")}
        host = engine.loop_host_stats()            # the host thread's side of the timed fits (dense loops)
        pair_us = event_pair_overhead_us()         # what a HIP-event pair around nothing reads: every timed scope over-reads by it
        pen_work = engine.pen_work_get() if pen else None      # device counts over the timed region: grid entries, ordered pairs, columns
    # configs[3]'s per-GPU job on THIS GPU (N = 1 only): 1 024 frames of the same generator through the default column pool, so that
    # a 1 -> N curve read off the driver's lines divides equal jobs (the N > 1 lines fit 1 024 frames per GPU and carry
    # `single_gpu_same_job_frames_per_s`; this is the same figure measured in the N = 1 run)
    configs3 = None
    if world == 1 and not (full or pen) and not args.no_configs3 and B != 1024 and args.lbs == "dense":
        n3 = 1024
        fr3 = synthetic.make_frames(n3, joints_fn, len(jm), start=0, focal=focal)

        def fit3():
            return driver.fit_frames(dm, cfg, fr3["keypoints"], jw, fr3["H"], fr3["W"], fr3["focal"], reg_pose=fr3["reg_pose"],
                                     reg_global=fr3["reg_global"], lbs_mode="dense", reuse_entry_eval=True, slots=-1)
        fit3()
        torch.cuda.synchronize()
        t3 = time.time()
        r3 = fit3()
        torch.cuda.synchronize()
        d3 = time.time() - t3
        ev3 = r3["stage_evals"].sum(1)
        configs3 = {"frames": n3, "gemm_columns": driver.auto_slots(n3) or n3, "frames_per_s": n3 / d3, "ms": 1e3 * d3,
                    "closure_evals_per_frame_mean": float(ev3.mean()), "closure_evals_per_frame_max": int(ev3.max())}
    # side key: the same job on the detector that keeps >= 3 of the 4 camera-initialisation keypoints (round 2's headline)
    side_min3 = None
    if not (full or pen) and not args.no_side:
        one_fit(fr=frames_min3)
        sync()
        t1 = time.time()
        for _ in range(args.steps):
            st_m3, _ = one_fit(fr=frames_min3)
        sync()
        dtm = all_max(time.time() - t1)
        ev3 = st_m3["stage_evals"].sum(1)
        side_min3 = {"value": world * B * args.steps / dtm, "ms_per_step": 1e3 * dtm / args.steps,
                     "closure_evals_per_frame_mean": float(ev3.mean()), "closure_evals_per_frame_max": int(ev3.max())}
        side_min3.update(loss_distribution(st_m3["stage_loss"][:, -1]))
    # the same job through the needed-rows path (what the product runs when nothing consumes the
    # full mesh inside the loop): one warm-up fit, then the same number of timed fits
    alt = None
    if args.lbs == "dense" and not args.no_alt and world == 1:
        one_fit("rows")
        sync()
        t1 = time.time()
        for _ in range(args.steps):
            st_alt, _ = one_fit("rows")
        sync()
        dta = all_max(time.time() - t1)
        alt = {"lbs_mode": "rows", "value": world * B * args.steps / dta, "unit": "frames/s",
               "ms_per_step": 1e3 * dta / args.steps,
               "closure_evals_per_frame_mean": float(st_alt["stage_evals"].sum(1).mean())}
        alt.update(loss_distribution(st_alt["stage_loss"][:, -1]))
        alt["paired_vs_dense"] = paired_stats(st_alt["stage_loss"][:, -1], st["stage_loss"][:, -1], "rows", "dense")
        alt["note"] = ("persistent per-frame kernel k_fit_rows: SMPL-X forward/adjoint on the rows the loss reads "
                       "(SURVEY 8d: legitimate while coll_loss_weight == 0); same objective, same optimiser; paired_vs_dense "
                       "compares the two paths' final losses frame by frame (the fits are chaotic: per-frame differences of "
                       "per cent are expected, the distributions must agree)")
    # per-rank report ("report per-GPU eval counts"): one small all_gather
    evals = st["stage_evals"].sum(1)
    ref_evals = st["stage_ref_evals"].sum(1)
    ranks = None
    if dist is not None:
        mine = torch.tensor([dt_rank, float(evals.mean()), float(evals.max()), float(evals.sum()), gather_ms[0],
                             float(np.nanmean(st["stage_loss"][:, -1]))], dtype=torch.float64, device=None if rehearsal else dev)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        ranks = [{"rank": r, "frames_per_s": B * args.steps / float(v[0]), "seconds": float(v[0]),
                  "closure_evals_per_frame_mean": float(v[1]), "closure_evals_per_frame_max": int(v[2]),
                  "closure_evals_total": int(v[3]), "gather_ms_last_step": float(v[4]), "final_loss_mean": float(v[5])}
                 for r, v in enumerate(x.cpu().numpy() for x in allr)]

    if rank == 0:
        tag = {"body": "configs[1]" if world == 1 else "configs[3]", "full": "configs[2]", "pen": "configs[4]"}[args.workload]
        what = {"body": "body-only K=25, camera + 5-stage L-BFGS (fit_smplx_smplifyx.yaml, use_vposer=False)",
                "full": "hands+face K=135, VPoser in the loop, camera + 5-stage L-BFGS (fit_smplx_smplifyx.yaml)",
                "pen": "fit_smplx_combined_halpe.yaml verbatim (K=136, interpenetration 128 / 1e-4), camera + 3 stages"}[args.workload]
        out = {
            "metric": "fitted frames/sec", "value": world * B * args.steps / dt, "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s: %d synthetic frames/GPU%s, %s" % (
                           tag, B, "" if world == 1 else " x %d GPUs, 1 RCCL all_gather/step" % world, what),
                       "model": "neutral SMPL-X-shaped synthetic model (seed 0%s); synthetic regression prior / VPoser weights as SURVEY 8(d)" % (
                           (", on the SMPL-X face topology, per-face part table and ExPose body of the reference tree (smplx_topology.npz)" if topo
                            else ", surface-like tube mesh + synthetic part labels") if pen else ""),
                       "keypoints": "SURVEY 8(d) verbatim: projected model joints + 1 px noise, confidences U(0.3, 1), 10 % of the keypoints "
                                    "dropped (the sequence of rounds 1-2a; `value_min3_camera_keypoints` = the same job when the detector "
                                    "keeps at least 3 of the 4 camera-initialisation keypoints, round 2's headline sequence)",
                       "frames_per_gpu": B, "lbs_mode": args.lbs,
                       "gemm_columns_per_gpu": (args.slots if (0 < args.slots < B and args.lbs == "dense") else B),
                       "parallelism": "frames sharded, dp%d" % world,
                       # N = 1: configs[3]'s per-GPU job (1 024 frames through the default column pool) fitted behind the headline --
                       # the denominator of a 1 -> N scaling curve on equal jobs (N > 1 lines: single_gpu_same_job_frames_per_s)
                       "configs3_single_gpu_frames_per_s": configs3["frames_per_s"] if configs3 else None,
                       "configs3_single_gpu": configs3,
                       "closure_evals_per_frame_mean": float(evals.mean()),
                       "closure_evals_per_frame_max": int(evals.max()),
                       # frames/s depends on how many evaluations a fit takes (a noisier closure stops earlier: round 1
                       # took 2 046 per frame and ended 3.4 % above the reference); evaluations/s is the engine's own rate
                       "closure_evals_per_s": float(world * args.steps * evals.sum() / dt) if world == 1 else None,
                       "reference_equiv_evals_per_frame_mean": float(ref_evals.mean()),
                       "arithmetic": "fp32 parameters, blend shapes, projection, losses, reverse sweep and optimiser (as the reference); "
                                     "fp64 inside the keypoint forward (rotations, kinematic chain, keypoint-vertex skinning), rounded "
                                     "to fp32 before the projection"},
        }
        out["config"].update(loss_distribution(st["stage_loss"][:, -1]))
        if ranks is not None:
            out["ranks"] = ranks
            out["config"]["closure_evals_per_s"] = float(sum(r["closure_evals_total"] for r in ranks) * args.steps / dt)
            # the per-GPU rate of THIS job size: a rank's own B frames over its own time, before it waits for the others.
            # rank 0's is a single-GPU run of the same job (frames are independent, no data-path collective), so scaling
            # efficiency on equal jobs is value / (n_gpus x single_gpu_same_job); the driver's N=1 line is configs[1]'s
            # smaller job (256 frames) and is not the denominator
            rates = [r["frames_per_s"] for r in ranks]
            out["config"].update(per_gpu_frames_per_s_min=min(rates), per_gpu_frames_per_s_mean=float(np.mean(rates)),
                                 single_gpu_same_job_frames_per_s=rates[0],
                                 per_gpu_closure_evals_max=max(r["closure_evals_per_frame_max"] for r in ranks),
                                 gather_ms_max=max(r["gather_ms_last_step"] for r in ranks))
        if not args.full:
            line = json.dumps(compact_line(out), allow_nan=False)
            assert len(line) < LINE_LIMIT and "\n" not in line, len(line)
            print(line, flush=True)
    if rank == 0 and args.full:
        ms_dense, n_dense, u_dense = prof["lbs_dense"]
        ms_clo, n_clo, u_clo = prof["tick"]
        ms_lb, n_lb, _ = prof["fit_rows"]
        out["kernels_ms_avg"] = {"lbs_dense": ms_dense / max(n_dense, 1), "tick_dense": ms_clo / max(n_clo, 1),
                                 "fit_rows": ms_lb / max(n_lb, 1),
                                 "penetration": prof["penetration"][0] / max(prof["penetration"][1], 1),
                                 "timed_launches_per_step": (n_dense + n_clo + n_lb) / max(args.steps, 1)}
        if host["rounds"]:
            # where a step's wall time goes on the host: its thread enqueues (hidden behind the GPU on a quick host), waits for the
            # stage flags of a finished batch (= the GPU is the bottleneck: good), or neither (the GPU starved: the loop's wall
            # time minus the kernels' time is then queue-dry time)
            k_us = 1e3 * (ms_dense / max(n_dense, 1) + ms_clo / max(n_clo, 1) + prof["penetration"][0] / max(prof["penetration"][1], 1))
            # a HIP-event pair around NOTHING on an idle stream reads this much (the timestamps sit in the command processor's
            # packet stream, not at the kernel's first and last wavefront): each of the round's timed scopes over-reads by it, which
            # made the scopes sum to MORE than the loop's wall time per round (round 4: 107.9 against 105.1 us) and pinned
            # queue_dry_frac at its clamp.  Measured here, subtracted from the per-round sum the host figures use.
            n_scopes = 2 + (1 if prof["penetration"][1] else 0)
            k_net = max(k_us - n_scopes * pair_us, 0.0)
            out["host"] = {"enqueue_us_per_round": 1e6 * host["enqueue_s"] / host["rounds"], "wait_frac": host["wait_s"] / max(host["wall_s"], 1e-12),
                           "loop_us_per_round": 1e6 * host["wall_s"] / host["rounds"], "kernels_us_per_round": k_net,
                           "kernels_us_per_round_events": k_us, "event_pair_us": pair_us,
                           "queue_dry_frac": max(0.0, 1.0 - k_net * host["rounds"] / max(1e6 * host["wall_s"], 1e-12)),
                           # what a step spends OUTSIDE the fitting loop (batch set-up on the host, result collection, the gather):
                           # ~15 ms on an idle host; hundreds of ms on a box whose host cores are taken -- the frames/s of such a run
                           # say nothing about the kernels (halpe workload, round 4: 272 and 362 against 467-487 frames/s)
                           "outside_loop_ms_per_step": 1e3 * (dt_rank - host["wall_s"]) / args.steps}
        if side_min3 is not None:
            out["value_min3_camera_keypoints"] = side_min3["value"]
            out["min3_camera_keypoints"] = side_min3
        # counter-derived figures are REPLAYED from the profile of the same command (one summary per workload: tools/run_prof.sh)
        pmc_name = "pmc_summary_full.json" if full else "pmc_summary_pen.json" if pen else "pmc_summary.json"
        pmc = os.path.join(ROOT, "profiles", pmc_name)
        pmc_ok, pmc_note = pmc_is_current(pmc)
        if pmc_ok and B != 256:     # (the counter passes run the default 256 frames per GPU: per-launch traffic of another job size is not theirs)
            pmc_ok, pmc_note = False, "profiles/%s was taken at 256 frames per GPU, this run has %d: traffic not replayed" % (pmc_name, B)
        pj = json.load(open(pmc)) if pmc_ok else {}

        def profiled_us(prefix, path=None, merge=False):
            """Average duration (us) of the kernel in the rocprofv3 --kernel-trace --stats summary of this command
            (profiles/kernel_stats*.csv, taken with the counters: same source hash), or None.  HIP events bracket the dispatch as
            well: they read 2-3 us longer than the profiler's own clock on a 55-us kernel."""
            import csv
            path = path or os.path.join(ROOT, "profiles", pmc_name.replace("pmc_summary", "kernel_stats").replace(".json", ".csv"))
            if not (pmc_ok and os.path.exists(path)):
                return None
            best, calls, tot = None, 0, 0.0
            for row in csv.DictReader(open(path)):
                if prefix in row["Name"]:
                    calls += int(row["Calls"]); tot += float(row["TotalDurationNs"]) * 1e-3
                    if best is None or int(row["Calls"]) > best[0]:
                        best = (int(row["Calls"]), float(row["AverageNs"]) * 1e-3)
            if merge:       # one kernel in several workgroup widths (k_lbs_dense16<W>): all of its launches
                return tot / calls if calls else None
            return best[1] if best else None

        def pmc_kernel(prefix):
            """the instantiation with the most launches whose name contains `prefix` (templates: k_tick_dense<FrameLDSx<32, false>, 1>)"""
            cands = [v for n, v in pj.items() if prefix in n and isinstance(v, dict) and "hbm_read_bytes_per_launch" in v]
            return max(cands, key=lambda v: v.get("FETCH_SIZE", {}).get("launches", 0)) if cands else {}
        if args.lbs == "dense" and n_dense:
            # active-frame compaction makes the frames per launch vary: achieved = total algorithmic
            # flops of all launches / total kernel time (HIP events on the launch stream)
            t_tot = 1e-3 * ms_dense
            fpl = u_dense / n_dense                       # mean frames per launch
            fl = u_dense * lbs_flops_per_frame(dm.V)
            by = n_dense * lbs_bytes_per_launch(0, dm.V) + u_dense * (lbs_bytes_per_launch(1, dm.V) - lbs_bytes_per_launch(0, dm.V))
            out["roofline"] = {"kernel": "k_lbs_dense16", "bound": "mfma", "achieved": fl / t_tot / 1e12,
                               "peak": PEAK_MFMA_F32 / 1e12, "unit": "TFLOP/s", "frac": fl / t_tot / PEAK_MFMA_F32,
                               "traffic": None, "flops_per_launch": fl / n_dense, "bytes_per_launch": by / n_dense,
                               "hbm_GBps": by / t_tot / 1e9, "hbm_frac": by / t_tot / PEAK_HBM,
                               "avg_launch_us": 1e6 * t_tot / n_dense, "launches": n_dense, "frames_per_launch": fpl,
                               "share_of_step": max(ms_dense - 1e-3 * pair_us * n_dense, 0.0) * args.prof_every / (1e3 * dt),
                               "launch_sampling": "HIP events around every %d-th launch over the whole timed region" % args.prof_every}
            W_ = model["weights"]
            tj = np.mean([((int((W_[i:i + 16] != 0).any(0).sum()) + 3) // 4) * 4 for i in range(0, dm.V, 16)])
            fle = u_dense * lbs_flops_executed_per_frame(dm.V, tj)
            out["roofline"].update({"achieved_executed": fle / t_tot / 1e12, "frac_executed": fle / t_tot / PEAK_MFMA_F32,
                                    "note": "achieved = SURVEY 8(d) algorithmic flops (dense 55-joint skinning product, 45.85 "
                                            "MFLOP/frame) / kernel time; achieved_executed counts only issued MFMA work "
                                            "(K padded to 512, skinning restricted to the %.1f joints per 16-vertex tile that "
                                            "carry weight); mfma_busy_frac = SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CYCLES of the profiled run" % tj})
            if not pmc_ok:
                out["roofline"]["traffic_note"] = pmc_note
            else:           # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command (tools/run_prof.sh)
                k = pmc_kernel("k_lbs_dense16")
                if "hbm_read_bytes_per_launch" in k and "hbm_write_bytes_per_launch" in k:
                    out["roofline"]["traffic"] = k["hbm_read_bytes_per_launch"] + k["hbm_write_bytes_per_launch"]
                    out["roofline"]["traffic_detail"] = {
                        "read_bytes_per_launch": k["hbm_read_bytes_per_launch"],
                        "write_bytes_per_launch": k["hbm_write_bytes_per_launch"],
                        "source": "replayed: profiles/" + pmc_name + ", the rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this "
                                  "command (tools/run_prof.sh; counters cannot be read inside an un-profiled run), FETCH_SIZE x2 "
                                  "per the gfx950 correction"}
                if "mfma_busy_frac" in k:
                    out["roofline"]["mfma_busy_frac"] = k["mfma_busy_frac"]
            out["roofline"]["avg_launch_us_profile"] = profiled_us("k_lbs_dense16", merge=True)
            # the other half of the step: loss + adjoint + L-BFGS tick + next pose / chain, one workgroup per frame.  Byte model
            # per launch (tick_bytes: shared once + per frame) from THIS workload's own numbers: the vertex items under the
            # keypoints that are live in a stage (body | + hands | all; fit_single_frame.py:569-572), weighted by the evaluations
            # the run spent in each stage; the live optimiser variables; the VPoser decoder's weights when it is in the loop
            if n_clo:
                nbj = engine.NUM_BODY_JOINTS[cfg.get("format", "coco25")]
                n_extra = len(model.get("extra_vertex_ids", engine.SMPLX_EXTRA_VERTEX_IDS))
                rows_cls, dyn_cls = item_rows_by_class(jm, n_extra, int(np.asarray(model["lmk_faces_idx"]).shape[0]), nbj)
                sw_list, _ = engine.stage_weights_from_cfg(cfg)
                cls_of = [2 if w.face_joint_weight != 0 else (1 if w.hand_joint_weight != 0 else 0) for w in sw_list]
                ev_stage = st["stage_evals"].sum(0).astype(np.float64)           # [1 + stages]: camera stage first (all keypoints projected, 4 weighted)
                wts = np.array([ev_stage[0]] + [ev_stage[1 + i] for i in range(len(cls_of))])
                mean_over = lambda per_cls: float((wts * np.array([per_cls[2]] + [per_cls[c] for c in cls_of], np.float64)).sum() / max(wts.sum(), 1.0))
                rows_live, rows_dyn = mean_over(rows_cls), mean_over(dyn_cls)
                use_vp = bool(cfg.get("use_vposer", True))
                n_live = (32 if use_vp else 63) + 3 + 10 + 3 + (24 + 3 + 3 + 3 + 10)          # embedding, orient, betas, cam | hands, jaw, eyes, expression
                vp_bytes = 4.0 * (512 * 32 + 512 * 512 + 126 * 512 + 512 + 512 + 126) if use_vp else 0.0
                by_shared, by_frame = tick_bytes(rows_live - rows_dyn, rows_dyn, n_live, use_vp, vp_bytes)
                t_clo = 1e-3 * ms_clo
                act = u_clo if u_clo else fpl * n_clo
                by_launch = by_shared + by_frame * act / n_clo
                out["roofline_tick"] = {"kernel": "k_tick_dense", "bound": "hbm", "achieved": by_launch * n_clo / t_clo / 1e9,
                                        "peak": PEAK_HBM / 1e9, "unit": "GB/s", "frac": by_launch * n_clo / t_clo / PEAK_HBM,
                                        "traffic": None, "bytes_per_frame_launch": by_frame, "rows_per_frame_launch": rows_live,
                                        "bytes_per_launch": by_launch, "shared_bytes_per_launch": by_shared,
                                        "avg_launch_us": 1e6 * t_clo / n_clo,
                                        "launches": n_clo, "frames_per_launch": act / n_clo,
                                        "share_of_step": max(ms_clo - 1e-3 * pair_us * n_clo, 0.0) * args.prof_every / (1e3 * dt),
                                        # what one frame pulls through its compute unit's L2 port per launch, and the rate that is over
                                        # the launch (a CU streams ~100 GB/s from L2: tools/micro/stream_cu.hip)
                                        "l2_stream_bytes_per_frame": by_shared + by_frame,
                                        "l2_stream_GBps_per_cu": (by_shared + by_frame) * n_clo / t_clo / 1e9,
                                        "rows_by_stage_class": rows_cls, "dynamic_rows_by_stage_class": dyn_cls, "live_variables": n_live,
                                        "vposer_weight_bytes": vp_bytes,
                                        "note": "latency-bound by construction (one frame's serial L-BFGS chain per workgroup): the "
                                                "figure to watch is avg_launch_us.  bytes_per_launch = constants every frame shares (static "
                                                "adjoint rows, 2 x VPoser weights: once per launch, as the GEMM's matrix) + per frame "
                                                "(dynamic-contour rows, history, vectors) x frames, rows evaluation-weighted over the stages"}
                out["roofline_tick"]["avg_launch_us_profile"] = profiled_us("k_tick_dense")
                if pmc_ok:
                    k = pmc_kernel("k_tick_dense")
                    if "hbm_read_bytes_per_launch" in k:
                        out["roofline_tick"]["traffic"] = k["hbm_read_bytes_per_launch"] + k.get("hbm_write_bytes_per_launch", 0.0)
                        out["roofline_tick"]["traffic_source"] = "replayed: profiles/" + pmc_name
        else:
            # persistent per-frame kernel: bytes the needed-rows closure must move per evaluation
            # (11 vertex rows x (3 x 506 blend-shape + 8 skinning entries), forward and adjoint)
            rows = 11
            by_eval = rows * (3 * 506 + 16) * 4.0 * 2
            total_evals = float(evals.sum()) * args.steps
            t_tot = 1e-3 * ms_lb
            out["roofline"] = {"kernel": "k_fit_rows", "bound": "hbm", "achieved": by_eval * total_evals / max(t_tot, 1e-12) / 1e9,
                               "peak": PEAK_HBM / 1e9, "unit": "GB/s", "frac": by_eval * total_evals / max(t_tot, 1e-12) / PEAK_HBM,
                               "traffic": None, "bytes_per_eval": by_eval, "evals": total_evals,
                               "kernel_ms_total": ms_lb, "launches": n_lb, "bytes_per_launch": by_eval * total_evals / max(n_lb, 1),
                               "note": "latency-bound by construction: one workgroup walks one frame's serial "
                                       "L-BFGS chain; the meaningful figure is frames/s"}
            pmc_rows = os.path.join(ROOT, "profiles", "pmc_summary_rows.json")
            pmc_ok, pmc_note = pmc_is_current(pmc_rows)
            if pmc_ok and B != 256:
                pmc_ok, pmc_note = False, "profiles/pmc_summary_rows.json was taken at 256 frames per GPU, this run has %d: traffic not replayed" % B
            if pmc_ok:      # per LAUNCH of the persistent kernel (one launch = the whole fit of a batch stage range)
                cands = [v for n, v in json.load(open(pmc_rows)).items() if "k_fit_rows" in n and "hbm_read_bytes_per_launch" in v]
                if cands:
                    k = max(cands, key=lambda v: v.get("FETCH_SIZE", {}).get("launches", 0))
                    out["roofline"]["traffic"] = k["hbm_read_bytes_per_launch"] + k.get("hbm_write_bytes_per_launch", 0.0)
                    out["roofline"]["traffic_source"] = "replayed: profiles/pmc_summary_rows.json (per launch of k_fit_rows)"
            else:
                out["roofline"]["traffic_note"] = pmc_note
        if pen and prof["penetration"][1]:
            # the interpenetration step of a round (csrc/collide.hip k_pen_* + the dense skinning adjoint, csrc/lbs_adjoint.hip), timed
            # as ONE HIP-event scope per round.  Byte model per GEMM column whose stage carries a collision weight (F triangles, V
            # vertices, E grid entries, P ordered pairs -- E and P are COUNTED on the device over the timed region,
            # engine.pen_work_get): broad phase = vertices 12 V + faces 12 F + part labels 4 F read, boxes 24 F written and read
            # back by the pair tests, entries 8 E written + (8 + 36) E read; narrow phase = pair list 8 P written and read, 2 x 36 B
            # of geometry per pair read, 40 B per pair of per-pair results written and read, per-triangle sums 40 F, vertex gradient
            # 12 V written; adjoint = d v_posed 12 V written and read by the fp32-MFMA GEMM (whose 63.7 MB of blend-shape rows are
            # shared by the launch: not in the per-column figure).
            ms_p, n_p, u_p = prof["penetration"]
            V_, F_ = dm.V, dm.F
            E_, P_, cols = pen_work["entries_per_column"], pen_work["pairs_per_column"], pen_work["columns"]
            by_col = (12 * V_ + 12 * F_ + 4 * F_ + 2 * 24 * F_ + (8 + 8 + 36) * E_) + (2 * 8 * P_ + 72 * P_ + 2 * 40 * P_ + 40 * F_ + 12 * V_) + 2 * 12 * V_
            t_p = 1e-3 * ms_p
            # columns that carried a collision weight per timed scope: counted on the device (cols over all scopes of the
            # timed region) -- the scope's `units` are all active columns, with or without the weight
            n_scopes_all = max(n_p * args.prof_every, 1)
            want_per_launch = cols / n_scopes_all
            out["roofline_pen"] = {"kernel": "k_pen_* + k_adj_* (one HIP-event scope per round)",
                                   "bound": "hbm", "achieved": by_col * want_per_launch * n_p / t_p / 1e9, "peak": PEAK_HBM / 1e9, "unit": "GB/s",
                                   "frac": by_col * want_per_launch * n_p / t_p / PEAK_HBM, "traffic": None, "bytes_per_column_launch": by_col,
                                   "avg_launch_us": 1e6 * t_p / n_p, "launches": n_p, "columns_per_launch": want_per_launch,
                                   "active_columns_per_launch": u_p / n_p,
                                   "grid_entries_per_column": E_, "pairs_per_column": P_,
                                   "share_of_step": max(ms_p - 1e-3 * pair_us * n_p, 0.0) * args.prof_every / (1e3 * dt),
                                   "bytes_per_launch": by_col * want_per_launch,
                                   "launches_per_round": int(driver.last_pen_launches),
                                   "lists_rederived_per_launch": pen_work["lists_overflowed"] / n_scopes_all,
                                   "walks_cut": pen_work["walks_cut"],
                                   "note": "dependent kernels of one round (launches_per_round: counted on the captured graph); bound by wavefront slots x dependent "
                                           "round trips, not by bytes (LAB_NOTES §4.6: two chains side by side take what one takes); E and P "
                                           "are device counts over the timed region; per-kernel times and counters: profiles/r06_pen_*"}
            if pmc_ok:
                tr = sum(v.get("hbm_read_bytes_per_launch", 0.0) + v.get("hbm_write_bytes_per_launch", 0.0) for k, v in pj.items()
                         if isinstance(v, dict) and k.startswith(("k_pen_", "k_adj_", "k_lbs_dense_adj")))
                out["roofline_pen"]["traffic"] = tr
                out["roofline_pen"]["traffic_source"] = "replayed: profiles/pmc_summary_pen.json (sum over the scope's kernels, FETCH_SIZE x 2 + WRITE_SIZE)"
            else:
                out["roofline_pen"]["traffic_note"] = pmc_note
        if alt is not None:
            out["alt"] = alt
        if not args.no_parity and not full and not pen and world == 1:
            try:
                out["reference_parity"] = reference_parity(model, args.lbs, raw=True)
                if side_min3 is not None:
                    out["min3_camera_keypoints"]["reference_parity"] = reference_parity(model, args.lbs, raw=False)
            except Exception as e:
                out["reference_parity"] = {"error": repr(e)}
        if not args.no_parity and pen and topo and world == 1:
            try:
                out["reference_parity"] = reference_parity_pen(dm, cfg, args.lbs)
            except Exception as e:
                out["reference_parity"] = {"error": repr(e)}
        if not args.no_parity and world == 1:
            try:
                out["closure_parity"] = closure_parity(model, args.workload, args.lbs)
            except Exception as e:
                out["closure_parity"] = {"error": repr(e)}
        if cpu_meas is not None:
            out["cpu_baseline"] = cpu_baseline_report(cpu_meas, float(ref_evals.mean())) if "error" not in cpu_meas \
                else {"value": None, "error": cpu_meas["error"]}
        dtag = args.workload + ("" if args.lbs == "dense" else "_" + args.lbs) + ("" if world == 1 else "_n%d" % world) + \
            ("" if B in (256, 1024) and not args.slots else "_f%d" % B + ("_s%d" % args.slots if args.slots else ""))
        out["detail"] = write_detail(out, dtag)
        line = json.dumps(compact_line(out), allow_nan=False)
        assert len(line) < LINE_LIMIT and "\n" not in line, len(line)
        print(line, flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
