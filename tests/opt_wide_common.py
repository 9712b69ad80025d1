"""Shared by test_opt_wide_host.py (CPU) and test_gpu_opt_wide.py (GPU): the configurations of the wide device optimiser
(sfx_opt_wide_*, engine.WideOptimizer: one workgroup per problem, up to 32768 variables) and the reference's own trajectories at
such sizes.  Objective family, arithmetic variants, lock-step replay, error measure and bound are those of opt_ext_common.py,
unchanged: bound = 10 x the larger error of the machine's two arithmetic variants on the same configuration, floor 1e-6."""
import os

import numpy as np
import torch

import opt_ext_common as X
from oracle.lbfgs_machine import StageMachine

NMAX = 32768            # SFX_WIDE_NMAX
MAX_GROUPS = 256        # SFX_WIDE_MAX_GROUPS
# (N, hyper-parameters): 193 the first size above the narrow limit; 4096 / 4097 either side of one 16-byte chunk per thread; 5003
# no multiple of 4; 32768 the cap; 3 and 65: most threads own nothing; hist9 wraps the ring.  The yardstick of a 32768
# configuration costs ~10 s of CPU: there are two.
WIDE_CONFIGS = [(193, "default"), (4096, "default"), (4097, "default"), (32768, "default"),
                (5003, "hist9"), (32768, "hist9"), (4097, "short"), (4097, "zero_tol"),
                (3, "zero_tol"), (65, "default")]
# what tests/lbfgs_wide_check.cpp (the header's machine over a serial vector layer) is run on, besides X.NAN_CONFIG
CHECK_CONFIGS = [(193, "default"), (5003, "hist9"), (4097, "short"), (4097, "zero_tol")]
INDEPENDENCE_CONFIG = (4097, "default")

GOLDEN_NS = (193, 1000)
GOLDEN_HYPER = X.GOLDEN_HYPER      # gen_lbfgs_wide: create_optimizer('lbfgsls', lr=1, maxiters=30)


def gold():
    """tests/golden/lbfgs_wide.npz (tools/make_goldens.py gen_lbfgs_wide): float32 runs of the real reference."""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbfgs_wide.npz"))


def golden_fn(x):
    a = ((torch.arange(x.numel()) % 10 + 1) ** 2).to(torch.float32)
    return 0.5 * (a * (x - 0.3) ** 2).sum() + 0.1 * torch.sin(3 * x).sum()


_GOLD_EVALS = {}


def golden_evals(N):
    """(xs, fs, gs) of the golden's run: g_k from CPU torch fp32 at the stored points; f_k must be the stored loss."""
    if N not in _GOLD_EVALS:
        g = gold()
        xs, fs, gs = [], [], []
        for pt, loss in zip(g["%d_points" % N], g["%d_losses" % N]):
            x = torch.tensor(pt, dtype=torch.float32, requires_grad=True)
            l = golden_fn(x)
            l.backward()
            assert np.float32(l.item()) == loss, (N, float(l.item()), loss)
            xs.append(pt.copy()); fs.append(np.float32(loss)); gs.append(x.grad.numpy().copy())
        _GOLD_EVALS[N] = (xs, fs, gs)
    return _GOLD_EVALS[N]


_GOLD_YARD = {}


def golden_yardstick(N):
    """[(variant, error against the golden's points, lock-step, same result)] for the plain machine and the two variants."""
    if N not in _GOLD_YARD:
        g = gold()
        xs, fs, gs = golden_evals(N)
        x0, res = g["%d_x0" % N], float(g["%d_res" % N])
        out = []
        for name, m in [("machine", StageMachine(x0, dtype=np.float32, **GOLDEN_HYPER))] + X.variants(x0, **GOLDEN_HYPER):
            err, lock = X.replay_against_points(m, xs, fs, gs)
            out.append((name, err, lock, X.same_result(m.result, res)))
        _GOLD_YARD[N] = out
    return _GOLD_YARD[N]


def golden_bound(N):
    return max(X.FLOOR, 10.0 * max(e[1] for e in golden_yardstick(N) if e[0] != "machine"))

