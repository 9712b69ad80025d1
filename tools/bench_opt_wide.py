"""Times of the wide device optimiser (sfx_opt_wide_*, engine.WideOptimizer, LBFGS(wide=True)).

1. Time per tick (one sfx_opt_wide_tell = one launch of B workgroups), split into line-search ticks (a trial point is consumed, the
   next one proposed) and iteration-head ticks (a line search ends: new pair, two-loop recursion over the FULL history of 100 pairs,
   first trial point), at (B, N) = (1, 4096), (1, 32768), (64, 4096).  The evaluations come from an ill-conditioned quadratic
   (a_i = 10^(6 i / N)), which keeps L-BFGS iterating long after the history has filled; ticks are timed with device events, one
   by one, after the 105th line search.  Beside the time: the bytes an iteration head has to move by the algorithm's own count
   (the recursion reads every stored s and y twice: 4 m N floats).
2. Wall time per closure evaluation of LBFGS(wide=True).step on the tests' objective family at N = 17674 (one shape over a clip of
   256 frames) and 31425 (per-vertex offsets), beside torch.optim.LBFGS(line_search_fn='strong_wolfe', history_size=100) on the
   same GPU closure, in the same process, the two alternating.  The two algorithms differ in details (torch's strong-Wolfe search is
   not the reference's): time per evaluation and evaluations are reported, not a claim of identical work.

usage: python tools/bench_opt_wide.py [--out profiles/opt_wide.json]
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

from smplifyx_amd import _capi as capi, engine            # noqa: E402
from smplifyx_amd.optimizers.lbfgs_ls import LBFGS        # noqa: E402

HIST, FULL_AFTER, LS_WANTED, TICK_LIMIT = 100, 105, 260, 1200
ROUNDS = 3


def tick_times(B, N, dev):
    a = torch.pow(10.0, 6.0 * torch.arange(N, device=dev, dtype=torch.float32) / N)
    x0 = torch.tensor(np.random.RandomState(1).uniform(-1, 1, (B, N)).astype(np.float32), device=dev)
    opt = engine.WideOptimizer(B, N, maxiters=1, ftol=0.0, gtol=0.0, max_iter=100000, max_eval=1000000, history_size=HIST,
                               tolerance_grad=0.0, tolerance_change=0.0)
    opt.trace(4096)
    cnt, prev = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for warm in (True, False):
        xt = opt.begin(x0)
        prev[:] = 0
        ls, head = [], []
        for k in range(60 if warm else TICK_LIMIT):
            g = a * xt
            f = 0.5 * (g * xt).sum(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.tell(f, g)
            e1.record()
            e1.synchronize()
            opt._call("get_trace", None, capi.iptr(cnt))
            ended = cnt - prev
            prev[:] = cnt
            if cnt.min() >= FULL_AFTER:      # every problem's history is full
                if ended.all():
                    head.append(e0.elapsed_time(e1) * 1e3)
                elif not ended.any():
                    ls.append(e0.elapsed_time(e1) * 1e3)
            if cnt.min() >= LS_WANTED or opt.active() == 0:
                break
    opt.close()
    med = lambda v: float(np.median(v)) if v else None
    return dict(B=B, N=N, history=HIST, line_search_tick_us=med(ls), line_search_ticks=len(ls), iteration_head_tick_us=med(head),
                iteration_head_ticks=len(head), iteration_head_bytes_per_problem=4 * HIST * N * 4,
                note="iteration-head bytes: the two-loop recursion's reads alone (s and y rows, each twice)")


def family_closure(x):
    N = x.numel()
    a = ((torch.arange(N, device=x.device) % 10 + 1) ** 2).to(torch.float32)

    def closure():
        x.grad = None
        loss = 0.5 * (a * (x - 0.3) ** 2).sum() + 0.1 * torch.sin(3 * x).sum()
        loss.backward()
        closure.n += 1
        return loss
    closure.n = 0
    return closure


def step_wall(N, dev):
    x0 = torch.tensor(np.random.RandomState(N).uniform(-1, 1, N).astype(np.float32), device=dev)
    out = dict(N=N, wide=[], torch=[])
    for r in range(ROUNDS + 1):          # (round 0 warms both up)
        for name in ("wide", "torch"):
            x = x0.clone().requires_grad_(True)
            closure = family_closure(x)
            if name == "wide":
                opt = LBFGS([x], lr=1.0, max_iter=20, history_size=HIST, line_search_fn="strong_Wolfe", wide=True)
            else:
                opt = torch.optim.LBFGS([x], lr=1.0, max_iter=20, history_size=HIST, line_search_fn="strong_wolfe")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):           # three steps: the second and third resume the history
                opt.step(closure)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r > 0:
                out[name].append(dict(evaluations=closure.n, us_per_evaluation=1e6 * dt / closure.n, final_loss=float(closure().detach())))
    for name in ("wide", "torch"):
        out[name + "_us_per_evaluation_median"] = float(np.median([e["us_per_evaluation"] for e in out[name]]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opt_wide.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_opt_wide.py needs a GPU: the optimiser has no CPU fallback")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0),
               ticks=[tick_times(B, N, dev) for B, N in ((1, 4096), (1, 32768), (64, 4096))],
               steps=[step_wall(N, dev) for N in (17674, 31425)])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
