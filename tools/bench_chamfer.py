"""Rates of the chamfer term: sfx_chamfer_forward and sfx_chamfer_backward (csrc/chamfer.hip) next to
sfx_eval_nearest (csrc/evaluate.hip: the kernel the forward grew from, distances only) at the same sizes in the same process.
  (i)  B = 256, Na = Nb = 10 475      the size of profiles/evaluation_mi355x.json: the synthetic template plus noise, twice
  (ii) B = 16, Na = 10 475, Nb = 50 000      a scan: the template plus noise against a resampling of it plus noise
The three calls alternate REPS times after WARM warm-up rounds, each between two HIP events on the current stream, on buffers
made once (the library calls themselves: no allocation inside the timed region); medians are reported.  The yardstick of the
forward is sfx_eval_nearest's time in the same run (expected about 9/7 of it, accepted up to 1.5 x); the backward has no
earlier code to compare with and is recorded beside the forward.  The kernels' register / LDS / scratch figures come from a
device-only compile of the unit with -Rpass-analysis=kernel-resource-usage (--no-compile leaves them out).
Nothing is asserted; whether the forward's distances agree with sfx_eval_nearest's (1e-5 relative: that unit contracts to
fused multiply-adds, this one does not) is recorded.  Prints one JSON line.

usage: timeout 600 python tools/bench_chamfer.py [--out profiles/chamfer_mi355x.json] [--no-compile]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smplifyx_amd import _args as A, _capi, engine, synthetic  # noqa: E402

REPS, WARM = 20, 3
SIZES = (("B256_mesh_mesh", 256, 10475), ("B16_mesh_scan", 16, 50000))
CSRC = os.path.join(ROOT, "smplify-x-partial_amd", "csrc")


def kernel_resources():
    """{kernel: {vgprs, sgprs, lds_bytes, scratch_bytes_per_lane, occupancy_waves_per_simd}} of csrc/chamfer.hip for gfx950."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "chamfer.hip"),
                            "-o", os.path.join(tmp, "chamfer.o")], capture_output=True, text=True, check=True)
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "LDS Size [bytes/block]": "lds_bytes",
            "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _Z\d+(k_chamfer_[a-z]+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for k, short in keys.items():
            m = re.search(r"\s%s: (\d+)" % re.escape(k), line)
            if m and name:
                out[name][short] = int(m.group(1))
    return out


def make_sets(B, Nb, seed=0):
    rng = np.random.RandomState(seed)
    v = np.asarray(synthetic.make_synthetic_model(0)["v_template"], np.float32)
    a = v[None] + (0.004 * rng.normal(size=(B,) + v.shape)).astype(np.float32)
    pick = rng.randint(0, v.shape[0], size=(B, Nb))
    b = v[pick] + (0.004 * rng.normal(size=(B, Nb, 3))).astype(np.float32)
    return torch.tensor(a).cuda(), torch.tensor(b).cuda()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)), reps=len(t))


def run_size(B, Nb, rho):
    lib = _capi.load()
    a, b = make_sets(B, Nb)
    Na, dev = a.shape[1], a.device
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    dab, dba, iab, iba, sab, sba = f32(B, Na), f32(B, Nb), i32(B, Na), i32(B, Nb), f32(B, Na), f32(B, Nb)
    loss, valid, da, db = f32(B, 2), i32(B, 2), f32(B, Na, 3), f32(B, Nb, 3)
    grad = torch.ones(B, 2, device=dev)
    nf, nb = engine.chamfer_forward_scratch_bytes(B, Na, Nb), engine.chamfer_backward_scratch_bytes(B, Na, Nb)
    sf, sb = torch.empty(nf // 4, dtype=torch.int32, device=dev), torch.empty(nb // 4, dtype=torch.int32, device=dev)
    p, st = A.ptr, A.stream(None, dev)
    calls = dict(
        eval_nearest=lambda: _capi.check(lib.sfx_eval_nearest(B, Na, Nb, p(a), p(b), None, None, 0, None, p(dab), p(dba), None, None, None, st)),
        chamfer_forward=lambda: _capi.check(lib.sfx_chamfer_forward(B, Na, Nb, p(a), p(b), None, None, None, None, rho, p(iab), p(iba),
                                                                    p(sab), p(sba), p(loss), p(valid), p(sf), nf, st)),
        chamfer_backward=lambda: _capi.check(lib.sfx_chamfer_backward(B, Na, Nb, p(a), p(b), None, None, None, None, rho, p(iab), p(iba),
                                                                      p(grad), p(da), p(db), p(sb), nb, st)))
    times = {k: [] for k in calls}
    for r in range(WARM + REPS):
        for k, fn in calls.items():                           # the three alternate
            t = timed(fn)
            if r >= WARM:
                times[k].append(t)
    agree = bool(torch.allclose(sab.sqrt(), dab, rtol=1e-5, atol=1e-7) and torch.allclose(sba.sqrt(), dba, rtol=1e-5, atol=1e-7))
    lens = torch.bincount(iba.reshape(-1).long().clamp(min=0) + Na * torch.arange(B, device=dev).repeat_interleave(Nb), minlength=B * Na)
    res = {k: stats(v) for k, v in times.items()}
    fwd = res["chamfer_forward"]["median_ms"]
    res.update(B=B, Na=Na, Nb=Nb, rho=rho, distances_agree_with_eval_nearest=agree,
               forward_over_eval_nearest=fwd / res["eval_nearest"]["median_ms"],
               backward_over_forward=res["chamfer_backward"]["median_ms"] / fwd,
               forward_distance_evaluations_per_s=2.0 * B * Na * Nb / (fwd * 1e-3),
               scatter_list_length_into_a=dict(median=float(lens.float().median()), max=int(lens.max())),
               scratch_bytes=dict(forward=nf, backward=nb))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rho", type=float, default=0.05)
    ap.add_argument("--no-compile", action="store_true")
    a = ap.parse_args()
    resources = None if a.no_compile else kernel_resources()   # (before the GPU is touched)
    assert torch.cuda.is_available(), "the device path needs a GPU: there is no CPU fallback"
    res = dict(bench="chamfer", device=torch.cuda.get_device_name(0), reps=REPS, warmup=WARM,
               scatter="inverted index per call (integer counts, exclusive scan, fill, rank placement); no O(Na Nb) sweep",
               kernel_resources=resources if resources is not None else "not measured",
               sizes={name: run_size(B, Nb, a.rho) for name, B, Nb in SIZES})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
