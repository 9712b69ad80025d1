"""Rates of the point-to-triangle term: sfx_p2m_forward and sfx_p2m_backward (csrc/p2m.hip) next to
sfx_chamfer_forward (csrc/chamfer.hip: the kernel the forward is shaped after, point-to-point) on the same B and Np with
Nb = Nv, in the same process.
  (i)  B = 256, Np = 10 475     a cloud of the mesh's own size
  (ii) B = 16, Np = 50 000      a scan
both against 10 475 vertices and 20 908 faces: the real SMPL-X topology when tests/golden/smplx_topology.npz is present, else the
synthetic model's faces.  The mesh is the synthetic template plus noise, the cloud a resampling of its vertices plus noise.
The three calls alternate REPS times after WARM warm-up rounds, each between two HIP events on the current stream, on buffers
made once (the library calls themselves: no allocation inside the timed region); medians are reported.
The yardstick of the forward is sfx_chamfer_forward's time in the same run.  Per (point, face) pair the inner loop of
k_p2m_nearest issues VALU_PER_PAIR["p2m"] vector instructions, per (point, point) pair that of k_chamfer_nearest
VALU_PER_PAIR["chamfer"] (counted by hand in the gfx950 disassembly of the two loops); sfx_chamfer_forward
evaluates B (Na Nb + Nb Na) pairs, sfx_p2m_forward B Np F.  Expected: time_p2m / time_chamfer = (Np F x p2m) / (2 Nv Np x
chamfer), accepted up to 1.5 x that.  The kernels' register / LDS / scratch figures come from a device-only compile of the unit
with -Rpass-analysis=kernel-resource-usage (--no-compile leaves them out).  Nothing is asserted.  Prints one JSON line.

usage: timeout 900 python tools/bench_p2m.py [--out profiles/p2m_mi355x.json] [--no-compile]
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
SIZES = (("B256_cloud_of_mesh_size", 256, 10475), ("B16_scan", 16, 50000))
CSRC = os.path.join(ROOT, "smplify-x-partial_amd", "csrc")
TOPOLOGY = os.path.join(ROOT, "tests", "golden", "smplx_topology.npz")
# vector instructions per pair in the two inner loops (DESIGN 4.12 says how they were counted)
VALU_PER_PAIR = dict(p2m=513 / 4.0, chamfer=124 / 16.0)
MARGIN = 1.5


def kernel_resources():
    """{kernel: {vgprs, sgprs, lds_bytes, scratch_bytes_per_lane, occupancy_waves_per_simd}} of csrc/p2m.hip for gfx950."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "p2m.hip"),
                            "-o", os.path.join(tmp, "p2m.o")], capture_output=True, text=True, check=True)
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "LDS Size [bytes/block]": "lds_bytes",
            "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _Z\d+(k_p2m_[a-z_]+?)7P2mArgs", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for k, short in keys.items():
            m = re.search(r"\s%s: (\d+)" % re.escape(k), line)
            if m and name:
                out[name][short] = int(m.group(1))
    return out


def topology(Nv):
    """(faces int32 [F, 3], what they are)."""
    if os.path.exists(TOPOLOGY):
        z = np.load(TOPOLOGY)
        for key in z.files:
            f = np.asarray(z[key])
            if f.ndim == 2 and f.shape[1] == 3 and f.dtype.kind in "iu" and f.shape[0] > 10000 and f.max() < Nv:
                return f.astype(np.int32), "SMPL-X topology (tests/golden/smplx_topology.npz: %s)" % key
    return np.asarray(synthetic.make_synthetic_model(0)["f"]).astype(np.int32), "synthetic model"


def make_sets(B, Np, seed=0):
    rng = np.random.RandomState(seed)
    v = np.asarray(synthetic.make_synthetic_model(0)["v_template"], np.float32)
    mesh = v[None] + (0.004 * rng.normal(size=(B,) + v.shape)).astype(np.float32)
    pick = rng.randint(0, v.shape[0], size=(B, Np))
    cloud = v[pick] + (0.004 * rng.normal(size=(B, Np, 3))).astype(np.float32)
    return torch.tensor(cloud).cuda(), torch.tensor(mesh).cuda()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)), reps=len(t))


def run_size(B, Np, rho):
    lib = _capi.load()
    cloud, mesh = make_sets(B, Np)
    Nv, dev = mesh.shape[1], mesh.device
    faces_host, what = topology(Nv)
    F = faces_host.shape[0]
    faces = torch.as_tensor(faces_host, device=dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    face, bary, dist2, loss, valid = i32(B, Np), f32(B, Np, 3), f32(B, Np), f32(B), i32(B)
    dp, dv, grad = f32(B, Np, 3), f32(B, Nv, 3), torch.ones(B, device=dev)
    iab, iba, sab, sba, closs, cvalid = i32(B, Nv), i32(B, Np), f32(B, Nv), f32(B, Np), f32(B, 2), i32(B, 2)
    nf, nb = engine.p2m_forward_scratch_bytes(B, Np, Nv), engine.p2m_backward_scratch_bytes(B, Np, Nv)
    nc = engine.chamfer_forward_scratch_bytes(B, Nv, Np)
    sf, sb, sc = (torch.empty(n // 4, dtype=torch.int32, device=dev) for n in (nf, nb, nc))
    p, st = A.ptr, A.stream(None, dev)
    calls = dict(
        chamfer_forward=lambda: _capi.check(lib.sfx_chamfer_forward(B, Nv, Np, p(mesh), p(cloud), None, None, None, None, rho, p(iab), p(iba),
                                                                    p(sab), p(sba), p(closs), p(cvalid), p(sc), nc, st)),
        p2m_forward=lambda: _capi.check(lib.sfx_p2m_forward(B, Np, Nv, F, p(cloud), p(mesh), p(faces), None, None, None, rho, p(face), p(bary),
                                                            p(dist2), p(loss), p(valid), p(sf), nf, st)),
        p2m_backward=lambda: _capi.check(lib.sfx_p2m_backward(B, Np, Nv, F, p(cloud), p(mesh), p(faces), None, None, rho, p(face), p(grad),
                                                              p(dp), p(dv), p(sb), nb, st)))
    times = {k: [] for k in calls}
    for r in range(WARM + REPS):
        for k, fn in calls.items():                           # the three alternate
            t = timed(fn)
            if r >= WARM:
                times[k].append(t)
    res = {k: stats(v) for k, v in times.items()}
    fwd, yard = res["p2m_forward"]["median_ms"], res["chamfer_forward"]["median_ms"]
    expected = (Np * F * VALU_PER_PAIR["p2m"]) / (2.0 * Nv * Np * VALU_PER_PAIR["chamfer"])
    lens = torch.bincount((faces[face.reshape(-1).long().clamp(min=0)].reshape(B, -1).long()
                           + Nv * torch.arange(B, device=dev)[:, None]).reshape(-1), minlength=B * Nv)
    res.update(B=B, Np=Np, Nv=Nv, F=F, rho=rho, topology=what,
               surface_not_farther_than_nearest_vertex=bool((dist2 <= sba * (1 + 1e-5) + 1e-12).all()),
               forward_over_chamfer_forward=fwd / yard, expected_ratio_from_valu_per_pair=expected, accepted_up_to=MARGIN * expected,
               within_margin=bool(fwd / yard <= MARGIN * expected),
               backward_over_forward=res["p2m_backward"]["median_ms"] / fwd,
               forward_pairs_per_s=float(B) * Np * F / (fwd * 1e-3),
               corner_list_length_per_vertex=dict(median=float(lens.float().median()), max=int(lens.max())),
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
    res = dict(bench="p2m", device=torch.cuda.get_device_name(0), reps=REPS, warmup=WARM, valu_per_pair=VALU_PER_PAIR, margin=MARGIN,
               kernel_resources=resources if resources is not None else "not measured",
               sizes={name: run_size(B, Np, a.rho) for name, B, Np in SIZES})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
