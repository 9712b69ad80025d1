"""Rendering rate of fitted meshes over their images: engine.render_meshes (csrc/raster.hip) for B = 256
bodies at 800 x 600 and at 1920 x 1080, kernel by kernel, next to the numpy oracle of the same contract (tests/raster_common.py) on
one body of the same shapes -- there is no other implementation on this machine to compare with (pyrender is not installed).
The bodies: the real SMPL-X surface of the topology fixture when it has been built (10 475 vertices, 20 908 faces), else the
synthetic tube model; each turned about y by its own angle and placed so that it fills about 80 % of the image height.
  device  torch.cuda.Event around REPS whole calls (rgba over a background image) after WARM warm-up calls; then the library's
          HIP-event profiler (engine.prof_enable) over REPS more calls for the pieces: render_clear (the visibility buffer's
          memset), render_project, render_vnormals, render_cover, render_resolve -- per batch of B, summed over the chunks the
          batch is walked in (max_pixels)
  oracle  RC.rasterize + RC.shade of body 0, wall clock, once per shape
Nothing is asserted but that device and oracle agree on body 0's coverage.  Prints one JSON line.

usage: python tools/bench_render.py [--B 256] [--out profiles/render_mi355x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from smplifyx_amd import engine, synthetic  # noqa: E402
import raster_common as RC  # noqa: E402

REPS, WARM = 10, 2
SHAPES = [(600, 800), (1080, 1920)]
PIECES = ("render_clear", "render_project", "render_vnormals", "render_cover", "render_resolve")


def make_bodies(B, seed=0):
    rng = np.random.RandomState(seed)
    if synthetic.topology_available():
        tp = synthetic.load_topology()
        v, f, what = np.asarray(tp["vertices"], np.float64), np.asarray(tp["faces"], np.int64), "SMPL-X surface (topology fixture)"
    else:
        m = synthetic.make_synthetic_model(0, surface=True)
        v, f, what = np.asarray(m["v_template"], np.float64), np.asarray(m["f"]).astype(np.int64), "synthetic tube model"
    v = v - (v.max(0) + v.min(0)) / 2.0
    out = np.empty((B,) + v.shape, np.float32)
    for b in range(B):
        a = rng.uniform(-np.pi, np.pi)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        out[b] = v @ Ry.T
    return out, f, float(np.ptp(v[:, 1])), what


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the device path needs a GPU: there is no CPU fallback"
    B = a.B
    verts, faces, height, what = make_bodies(B)
    V, F = verts.shape[1], faces.shape[0]
    d_verts = torch.tensor(verts).cuda()
    rng = np.random.RandomState(1)
    transl = np.stack([rng.uniform(-0.2, 0.2, B), rng.uniform(-0.05, 0.05, B), rng.uniform(2.8, 3.2, B)], 1).astype(np.float32)
    d_t = torch.tensor(transl).cuda()
    shapes = []
    for H, W in SHAPES:
        focal = 0.8 * H * 3.0 / height
        center = np.tile(np.array([W / 2.0, H / 2.0], np.float32), (B, 1))
        d_c = torch.tensor(center).cuda()
        bg = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")
        call = lambda want=("rgba",): engine.render_meshes(d_verts, faces, d_t, focal, d_c, H, W, background=bg, want=want)
        whole = device_ms(call)
        engine.prof_reset()
        engine.prof_enable(True)
        for _ in range(REPS):
            call()
        torch.cuda.synchronize()
        pieces = {}
        for name in PIECES:
            ms, n, _ = engine.prof_get(name)
            pieces[name] = dict(ms_per_batch=ms / REPS, launches_per_batch=n / float(REPS))
        engine.prof_enable(False)
        engine.prof_reset()
        out = call(want=("tri", "screen", "rgba"))
        tri = out["tri"]
        covered = (tri >= 0).sum(dim=(1, 2)).cpu().numpy()
        t0 = time.perf_counter()
        ras = RC.rasterize(out["screen"][0].cpu().numpy(), faces, H, W)
        _, _, ok = RC.snap(out["screen"][0].cpu().numpy())
        RC.shade(ras, RC.camera_points(verts[0].astype(np.float64), transl[0]), faces, ok)
        oracle_s = time.perf_counter() - t0
        same = bool(np.array_equal(tri[0].cpu().numpy() >= 0, ras["tri"] >= 0))
        chunk = max(1, min(B, engine.RENDER_MAX_PIXELS // (H * W)))
        shapes.append(dict(H=H, W=W, focal=focal, chunk_meshes=chunk, whole_call=whole, pieces=pieces,
                           pieces_sum_ms=sum(p["ms_per_batch"] for p in pieces.values()),
                           meshes_per_s=B / (whole["median_ms"] * 1e-3),
                           covered_pixels_per_mesh=dict(mean=float(covered.mean()), min=int(covered.min()), max=int(covered.max())),
                           hit_samples_body0=int(ras["hits"].sum()),
                           oracle_s_body0=oracle_s, oracle_s_per_batch_extrapolated=oracle_s * B,
                           ratio_oracle_over_device=oracle_s * B / (whole["median_ms"] * 1e-3),
                           coverage_agrees_body0=same))
        del bg, out, tri
        torch.cuda.empty_cache()
    res = dict(bench="render", device=torch.cuda.get_device_name(0), B=B, V=V, F=F, mesh=what,
               outputs="rgba over a uint8 background", shapes=shapes)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
