"""Shared by test_opt_ext_host.py (CPU) and test_gpu_opt_ext.py (GPU): the objective family, the arithmetic variants of
oracle/lbfgs_machine.StageMachine and the lock-step replay that the tests of the device optimiser for caller-supplied
evaluations (sfx_opt_*, engine.BatchOptimizer) are built on.

Replay.  An optimiser under test (the device, or a variant of the machine standing in for it) runs on a closure and every
evaluation it consumed is recorded: the point x_k it asked for and the (f_k, g_k) it was given.  The reference --
StageMachine(dtype=float32) -- is then fed THE SAME (f_k, g_k): before each feed its x_trial is compared with x_k.  No trajectory
passes through a second closure, so nothing chaotic separates the two; what remains is the rounding of the optimiser's own
arithmetic (dot products, axpys, the cubic interpolation) in one step.

Error measure: max |x_k - x_trial_machine| / max |x_trial_machine|, worst over the run.
Yardstick: that error for two arithmetic variants of the machine itself, each run on the CPU closure of the same configuration --
fma=False (the axpys rounded twice) and Dot64Machine (dot products accumulated in float64, rounded once).
Bound: 10 x the larger variant's error, floor 1e-6 (the suite's noise-floor constant, test_gpu_optimizer_steps._above_noise_floor)."""
import numpy as np
import torch

from oracle.lbfgs_machine import StageMachine, T

FLOOR = 1e-6

H_DEFAULT = dict()
H_HIST9 = dict(history=9)                                                           # wraps the ring, leaves a partial block of 8
H_SHORT = dict(maxiters=12, ftol=0.0, gtol=0.0, max_iter=7, max_eval=9, lr=0.5)     # every step cut short by max_iter / max_eval
H_ZERO_TOL = dict(maxiters=6, tol_grad=0.0, tol_change=0.0)                         # LBFGS's own tolerances switched off
NB = 5      # problems per batch: b = 0..4
# (N, hyper-parameters) the GPU tests run; the host test asserts the yardstick runs' lock-step for every one of them
GPU_CONFIGS = [(N, "default") for N in (1, 2, 3, 4, 64, 65, 191, 192)] + \
              [(N, h) for h in ("hist9", "short", "zero_tol") for N in (3, 65, 192)]
# the CPU check of the replay design looks at these as well
HOST_CONFIGS = GPU_CONFIGS + [(N, "default") for N in (10, 63)]
HYPER = dict(default=H_DEFAULT, hist9=H_HIST9, short=H_SHORT, zero_tol=H_ZERO_TOL)
# Batch independence: (N, hyper-parameters, how many different evaluation counts the 5 problems must end at).  N = 65, a full
# row and a bit: all five differ.  N = 3 (one lane; the configuration of the NaN case below): at least two -- the counts of so
# small a problem move with the last bit of the closure's sin / cos, which the CPU and the GPU do not share.
INDEPENDENCE_CONFIGS = [(65, "default", 5), (3, "zero_tol", 2)]
# The non-finite evaluation: problem NAN_PROBLEM of NAN_CONFIG gets NaN as its third loss (evaluation 2).  The case is chosen where
# the REFERENCE has a defined end: in most problems of the family the third evaluation meets the curvature condition, the
# reference then holds a one-point bracket whose `bracket_f[0] <= bracket_f[-1]` is false for NaN and indexes past it
# (lbfgs_ls.py:102-104, :163 -- an IndexError, in the machine as in the reference), so there is nothing to agree with.  Here the
# NaN lands in a two-point bracket, as an end that every comparison rejects, and the run goes on to a finite result.
NAN_CONFIG, NAN_PROBLEM, NAN_AT = (3, "zero_tol"), 4, 2


class Dot64Machine(StageMachine):
    """The machine with every dot product accumulated in float64 and rounded once."""

    def _dot(self, a, b):
        return T(np.dot(np.asarray(a, np.float64), np.asarray(b, np.float64)))


def variants(x0, **hyper):
    return [("fma=False", StageMachine(x0, dtype=np.float32, fma=False, **hyper)),
            ("dot64", Dot64Machine(x0, dtype=np.float32, **hyper))]


# ---- the objective family: f_b(x) = 0.5 sum a_i (x_i - (0.3 + 0.05 b))^2 + 0.1 sum sin(3 x_i), a_i = ((i mod 10) + 1)^2
def family_x0(N, b):
    return np.random.RandomState(100 * N + b).uniform(-1, 1, N).astype(np.float32)


def family_eval(x, b0=0):
    """x [B][N] float32 tensor (any device) -> (f [B], g [B][N]) of problems b0 .. b0 + B - 1, in float32 torch arithmetic."""
    B, N = x.shape
    a = ((torch.arange(N, device=x.device) % 10 + 1) ** 2).to(torch.float32)
    c = (0.3 + 0.05 * torch.arange(b0, b0 + B, device=x.device, dtype=torch.float32)).reshape(B, 1)
    d = x - c
    f = 0.5 * (a * d * d).sum(1) + 0.1 * torch.sin(3 * x).sum(1)
    g = a * d + 0.3 * torch.cos(3 * x)
    return f, g


def run_on_cpu_closure(m, b, nan_at=None):
    """Drive machine m on the CPU closure of problem b; returns the recorded run (xs, fs, gs).  nan_at = k: the loss of
    evaluation k is replaced by NaN."""
    xs, fs, gs = [], [], []
    while not m.done:
        x = m.x_trial.astype(np.float32).copy()
        f, g = family_eval(torch.from_numpy(x).reshape(1, -1), b)
        xs.append(x); fs.append(np.float32("nan") if len(fs) == nan_at else np.float32(f[0].item())); gs.append(g[0].numpy().copy())
        m.feed(fs[-1], gs[-1])
        assert len(xs) < 2000
    return xs, fs, gs


def replay(m, xs, fs, gs):
    """Feed the recorded evaluations to machine m.  Returns (worst relative difference of the trial points, lock-step): lock-step
    = m wanted every one of the evaluations and was done exactly after the last."""
    err = 0.0
    for x, f, g in zip(xs, fs, gs):
        if m.done:
            return err, False
        xm, xa = m.x_trial.astype(np.float64), np.asarray(x, np.float64)
        fin = np.isfinite(xm)          # (a run fed a non-finite loss may ask for non-finite points: the same ones, then)
        if not np.array_equal(fin, np.isfinite(xa)):
            return np.inf, False
        if fin.any():
            err = max(err, float(np.abs(xa[fin] - xm[fin]).max() / np.abs(xm[fin]).max()))
        m.feed(f, g)
    return err, bool(m.done)


def same_records(ra, rb):
    """Record sequences (machine.records / the device trace) of two runs in lock-step: the same types, the same evaluation
    counts per line search, per LBFGS.step and per run, the same result."""
    ra, rb = np.asarray(ra, np.float64).reshape(-1, 4), np.asarray(rb, np.float64).reshape(-1, 4)
    if ra.shape != rb.shape or not np.array_equal(ra[:, 0], rb[:, 0]):
        return False
    ls, st, fin = ra[:, 0] == 0, ra[:, 0] == 1, ra[:, 0] == 2
    return (np.array_equal(ra[ls, 3], rb[ls, 3]) and np.array_equal(ra[st, 2:], rb[st, 2:])
            and np.array_equal(ra[fin, 1].astype(np.float32), rb[fin, 1].astype(np.float32), equal_nan=True)
            and np.array_equal(ra[fin, 2], rb[fin, 2]))


def same_result(a, b):
    a = np.float32(np.nan if a is None else a); b = np.float32(np.nan if b is None else b)
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


_YARD = {}


def yardstick(N, hname, b):
    """Per problem of a configuration: [(variant, error, lock-step, same records, same result, evaluations)] of the two variants'
    own runs against the machine's replay.  Computed once per session."""
    key = (N, hname, b)
    if key not in _YARD:
        hyper, out = HYPER[hname], []
        for name, v in variants(family_x0(N, b), **hyper):
            xs, fs, gs = run_on_cpu_closure(v, b)
            m = StageMachine(family_x0(N, b), dtype=np.float32, **hyper)
            err, lock = replay(m, xs, fs, gs)
            out.append((name, err, lock, same_records(v.records, m.records), same_result(v.result, m.result), len(xs)))
        _YARD[key] = out
    return _YARD[key]


def bound(N, hname):
    """10 x the larger variant's error over the configuration's NB problems, floor 1e-6."""
    return max(FLOOR, 10.0 * max(e[1] for b in range(NB) for e in yardstick(N, hname, b)))


# ---- the reference's own trajectories (tests/golden/lbfgs.npz, made by tools/make_goldens.py gen_lbfgs)
def gold():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbfgs.npz"))


GOLDEN_CASES = [(f, N) for f in ("rosen", "quad") for N in (2, 6, 10)]


def golden_fn(fname, x):
    if fname == "rosen":
        return (100 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2).sum()
    a = torch.arange(1, x.numel() + 1, dtype=x.dtype, device=x.device) ** 2
    return 0.5 * (a * (x - 0.3) ** 2).sum() + 0.1 * torch.sin(3 * x).sum()


def golden_evals(g, fname, N):
    """(xs, fs, gs) of the golden's float32 run: f_k, g_k from CPU torch fp32 at the stored points; f_k must be the stored loss."""
    trace = g["%s_%d_f32_trace" % (fname, N)]
    xs, fs, gs = [], [], []
    for row in trace:
        x = torch.tensor(row[1:], dtype=torch.float32, requires_grad=True)
        assert np.array_equal(x.detach().numpy().astype(np.float64), row[1:]), "the golden's points are float32 values"
        l = golden_fn(fname, x)
        l.backward()
        assert float(l.item()) == row[0], (fname, N, float(l.item()), row[0])
        xs.append(x.detach().numpy().copy()); fs.append(np.float32(l.item())); gs.append(x.grad.numpy().copy())
    return xs, fs, gs


GOLDEN_HYPER = dict(maxiters=30, ftol=1e-9, gtol=1e-9, lr=1.0, max_iter=30)      # gen_lbfgs: create_optimizer('lbfgsls', maxiters=30)


def golden_yardstick(g, fname, N):
    """[(variant, error against the golden's points, lock-step, same result)] for the plain machine and the two variants, each fed
    the golden's evaluations."""
    xs, fs, gs = golden_evals(g, fname, N)
    x0 = g["%s_%d_f32_x0" % (fname, N)]
    res = float(g["%s_%d_f32_res" % (fname, N)])
    out = []
    for name, m in [("machine", StageMachine(x0, dtype=np.float32, **GOLDEN_HYPER))] + variants(x0, **GOLDEN_HYPER):
        err, lock = replay_against_points(m, xs, fs, gs)
        out.append((name, err, lock, same_result(m.result, res)))
    return out


def replay_against_points(m, xs, fs, gs):
    """As replay, with the RECORDED points as the reference of the error measure (the golden's trajectory is the reference)."""
    err = 0.0
    for x, f, gr in zip(xs, fs, gs):
        if m.done:
            return err, False
        xr = np.asarray(x, np.float64)
        err = max(err, float(np.abs(m.x_trial.astype(np.float64) - xr).max() / np.abs(xr).max()))
        m.feed(f, gr)
    return err, bool(m.done)


def golden_bound(g, fname, N):
    return max(FLOOR, 10.0 * max(e[1] for e in golden_yardstick(g, fname, N) if e[0] != "machine"))
