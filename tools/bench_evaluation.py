"""Scoring rate of fitted meshes: evaluation.compute_v2v on the device (csrc/evaluate.hip) next to the host
numpy / k-d tree path on the same meshes.  B = 256 meshes of V = 10 475: the synthetic model's template plus per-mesh noise as
ground truth, a similarity transform of it plus noise as the estimate.  Metrics: Procrustes-aligned vertex errors plus the F-score
at two thresholds (5 mm, 15 mm).
  device  torch.cuda.Event around REPS calls after WARM warm-up calls, per piece: engine.align_errors (Procrustes),
          engine.nearest_distances (two thresholds, counts only), and the whole compute_v2v(device=True)
  host    compute_v2v(device=False) on numpy copies: one thread over as many meshes as fit in --host-seconds / 3, then a pool
          of --threads threads (<= 16) for the rest of the budget; the device-to-host copy the host path needs is timed apart
Nothing is asserted but that both paths give the same F-scores on the first meshes.  Prints one JSON line.

usage: python tools/bench_evaluation.py [--B 256] [--host-seconds 30] [--threads 16] [--out profiles/evaluation_mi355x.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smplifyx_amd import engine, evaluation as E, synthetic  # noqa: E402

REPS, WARM = 20, 3
THRESHOLDS = [0.005, 0.015]


def make_meshes(B, seed=0):
    rng = np.random.RandomState(seed)
    v = np.asarray(synthetic.make_synthetic_model(0)["v_template"], np.float64)
    gt = v[None] + 0.004 * rng.normal(size=(B,) + v.shape)
    est = np.empty_like(gt)
    for b in range(B):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        est[b] = rng.uniform(0.8, 1.2) * gt[b] @ q.T + rng.normal(size=3) + 0.006 * rng.normal(size=v.shape)
    return est.astype(np.float32), gt.astype(np.float32)


def alignments():
    return {"procrustes": E.ProcrustesAlignmentMPJPE(fscore_thresholds=THRESHOLDS)}


def device_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(times)), min_ms=float(np.min(times)), max_ms=float(np.max(times)), reps=REPS)


def host_one(est, gt):
    return E.compute_v2v(est[None], gt[None], alignments())


def host_rate(est, gt, seconds, threads):
    """meshes / s of the host path: (one thread, a pool of `threads`); meshes are reused cyclically."""
    B = est.shape[0]
    t0, n1 = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds / 3.0:
        host_one(est[n1 % B], gt[n1 % B])
        n1 += 1
    one = n1 / (time.perf_counter() - t0)
    chunk = max(threads, int(one * threads))                 # about a second of work per round of the pool
    t0, nt = time.perf_counter(), 0
    with ThreadPoolExecutor(threads) as pool:
        while time.perf_counter() - t0 < seconds * 2.0 / 3.0:
            list(pool.map(lambda i: host_one(est[i % B], gt[i % B]), range(nt, nt + chunk)))
            nt += chunk
    return one, n1, nt / (time.perf_counter() - t0), nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--host-seconds", type=float, default=30.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the device path needs a GPU: there is no CPU fallback"
    threads = max(1, min(16, a.threads))
    est, gt = make_meshes(a.B)
    V = est.shape[1]
    d_est, d_gt = torch.tensor(est).cuda(), torch.tensor(gt).cuda()

    pieces = dict(
        align_procrustes=device_ms(lambda: engine.align_errors(d_est, d_gt, mode="procrustes")),
        nearest_two_thresholds=device_ms(lambda: engine.nearest_distances(d_est, d_gt, THRESHOLDS, return_distances=False)),
        compute_v2v_device=device_ms(lambda: E.compute_v2v(d_est, d_gt, alignments(), device=True)))
    copy = device_ms(lambda: (d_est.cpu(), d_gt.cpu()))

    # the two paths agree on what they score (first meshes; the F-scores come from integer counts)
    n_chk = min(2, a.B)
    dev = E.compute_v2v(d_est[:n_chk], d_gt[:n_chk], alignments(), device=True)
    ref = E.compute_v2v(est[:n_chk].astype(np.float64), gt[:n_chk].astype(np.float64), alignments())
    point_diff = float(np.abs(dev["point"]["procrustes"].cpu().numpy() - ref["point"]["procrustes"]).max())
    f_diff = max(float(np.abs(dev["fscore"]["procrustes"][t].cpu().numpy() - ref["fscore"]["procrustes"][t]).max()) for t in THRESHOLDS)

    one, n1, pooled, nt = host_rate(est, gt, a.host_seconds, threads)
    dev_rate = a.B / (pieces["compute_v2v_device"]["median_ms"] * 1e-3)
    pairs = 2.0 * a.B * V * V                                 # distance evaluations of one nearest call (both directions)
    res = dict(bench="evaluation", device=torch.cuda.get_device_name(0), B=a.B, V=V, thresholds=THRESHOLDS,
               metrics="Procrustes V2V + F-score at two thresholds", device_pieces=pieces,
               device_meshes_per_s=dev_rate,
               nearest_pair_evaluations_per_s=pairs / (pieces["nearest_two_thresholds"]["median_ms"] * 1e-3),
               device_to_host_copy=copy,
               host_one_thread_meshes_per_s=one, host_one_thread_meshes=n1,
               host_pool_threads=threads, host_pool_meshes_per_s=pooled, host_pool_meshes=nt,
               ratio_device_over_host_pool=dev_rate / pooled, ratio_device_over_host_one_thread=dev_rate / one,
               agreement=dict(meshes=n_chk, point_max_abs_diff=point_diff, fscore_max_abs_diff=f_diff,
                              fscore_host=[float(ref["fscore"]["procrustes"][t][0]) for t in THRESHOLDS]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
