"""Times of the stand-alone VPoser encoder: encode and encode + encode_backward of engine.VPoserEncoder next
to the same network as plain torch ops on the same GPU (oracle.vposer.VPoserEncoderRef in float32, backward by autograd) and
to the host route of the default VPoser.encode including its transfers.  Latent 32, n_in 63 and 189, B = 1 / 256 / 4096;
torch.cuda.Event after warm-up, median of 20, one process.  Prints one line per (n_in, B).

usage: python tools/vposer_encode_times.py
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.vposer import VPoserEncoderRef      # noqa: E402
from smplifyx_amd import engine, synthetic      # noqa: E402
from smplifyx_amd.vposer import VPoser          # noqa: E402

REPS, WARM = 20, 5


def matrot(pose):
    a = pose.reshape(-1, 3)
    ang = a.norm(dim=1, keepdim=True)
    u = a / ang
    z = torch.zeros_like(u[:, 0])
    K = torch.stack([z, -u[:, 2], u[:, 1], u[:, 2], z, -u[:, 0], -u[:, 1], u[:, 0], z], -1).view(-1, 3, 3)
    R = torch.eye(3, dtype=pose.dtype, device=pose.device)[None] + torch.sin(ang)[:, :, None] * K + (1 - torch.cos(ang))[:, :, None] * (K @ K)
    return R.reshape(pose.shape[0], 189)


def gpu_time(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def wall_time(fn):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def main():
    dev = torch.device("cuda:0")
    print("%5s %5s | %10s %12s | %10s %12s | %10s   (microseconds, median of %d)"
          % ("n_in", "B", "encode", "enc + bwd", "torch ops", "torch + bwd", "host route", REPS))
    for n_in in (63, 189):
        w = synthetic.make_synthetic_vposer(0, latent=32, encoder_inputs=n_in)
        enc = engine.VPoserEncoder(w)
        ref = VPoserEncoderRef(w, torch.float32).to(dev)
        host = VPoser(w).to(dev).eval()
        for B in (1, 256, 4096):
            rng = np.random.RandomState(B)
            pose = torch.tensor((0.3 * rng.normal(size=(B, 63))).astype(np.float32), device=dev)
            dm = torch.tensor(rng.normal(size=(B, 32)).astype(np.float32), device=dev)
            ds = torch.tensor(rng.normal(size=(B, 32)).astype(np.float32), device=dev)
            mean, sigma, dpose = torch.empty_like(dm), torch.empty_like(dm), torch.empty_like(pose)

            def fwd():
                enc.encode(pose, out_mean=mean, out_sigma=sigma)

            def both():
                enc.encode(pose, out_mean=mean, out_sigma=sigma)
                enc.encode_backward(pose, dm, ds, out=dpose)

            def t_fwd():
                with torch.no_grad():
                    q = ref.encode(matrot(pose) if n_in == 189 else pose)
                    return q.mean, q.stddev

            def t_both():
                p = pose.detach().requires_grad_(True)
                q = ref.encode(matrot(p) if n_in == 189 else p)
                ((q.mean * dm).sum() + (q.stddev * ds).sum()).backward()
                return p.grad

            print("%5d %5d | %10.1f %12.1f | %10.1f %12.1f | %10.1f"
                  % (n_in, B, gpu_time(fwd), gpu_time(both), gpu_time(t_fwd), gpu_time(t_both), wall_time(lambda: host.encode(pose))),
                  flush=True)
        enc.close()


if __name__ == "__main__":
    main()
