"""Shared by test_gpu_opt_ext.py and test_gpu_opt_wide.py: how the GPU tests of the two device optimisers for caller-supplied
evaluations (engine.BatchOptimizer, engine.WideOptimizer -- one Python class body, two handles) create a handle, drive it over
recorded evaluations and check a run against the machine; and the two tests that are the same test for both handles.  A handle
is named by its class in smplifyx_amd.engine (`cls`) and by the label its check_bound lines carry.  Reference, error measure,
yardstick and bound: tests/opt_ext_common.py."""
import numpy as np
import torch

import helpers as H
import opt_ext_common as X
from oracle.lbfgs_machine import StageMachine


def opt(cls, B, N, **hyper):
    from smplifyx_amd import engine
    return getattr(engine, cls)(B, N, **hyper)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def drive(opt, x0, evaluate, mode="fit", resume=False, extra=0, limit=400):
    """Run `opt` from x0 [B][N] (numpy) on evaluate(x_trial, k) -> (f [B], g [B][N]) CUDA tensors until no problem is active (+
    `extra` more evaluations).  Returns per evaluation the trial points, losses and gradients as numpy arrays, and the number of
    evaluations after which active() first read 0."""
    dev = opt.device
    xt = opt.begin(torch.tensor(x0, device=dev), mode=mode, resume=resume)
    xs, fs, gs, n_done = [], [], [], None
    k = 0
    while True:
        if n_done is None and opt.active() == 0:
            n_done = k
        if n_done is not None and k >= n_done + extra:
            break
        f, g = evaluate(xt, k)
        xs.append(xt.cpu().numpy().copy()); fs.append(f.cpu().numpy().copy()); gs.append(g.cpu().numpy().copy())
        opt.tell(f.contiguous(), g.contiguous())
        k += 1
        assert k < limit, "the device optimiser does not finish"
    return np.stack(xs), np.stack(fs), np.stack(gs), n_done


def family(b0=0):
    return lambda xt, k: X.family_eval(xt, b0)


def check_replay(label, what, hyper, x0, xs, fs, gs, res, trace, bound):
    """One problem's recorded run against the machine fed the same evaluations: the same number of evaluations (res['evals']),
    the same records, the same result, trial points within the bound."""
    n = int(res["evals"])
    m = StageMachine(x0, dtype=np.float32, **hyper)
    err, lock = X.replay(m, xs[:n], fs[:n], gs[:n])
    assert lock, (label, what, "the machine wants %s evaluations, the device consumed %d" % ("fewer" if m.done else "more", n))
    assert res["status"] == 1
    assert X.same_result(res["result"], m.result), (label, what, res["result"], m.result)
    if trace is not None:
        assert X.same_records(trace, m.records), (label, what, trace[:, 0], [r[0] for r in m.records])
    H.check_bound(label, what, err, bound)
    return err


_RUNS = {}


def family_run(cls, N, hname):
    """The batch of NB problems of a configuration on one handle, run once per session: (x0, xs, fs, gs, result, trace, n_done)."""
    key = (cls, N, hname)
    if key not in _RUNS:
        o = opt(cls, X.NB, N, **X.HYPER[hname])
        o.trace(256)
        x0 = np.stack([X.family_x0(N, b) for b in range(X.NB)])
        xs, fs, gs, n_done = drive(o, x0, family())
        r = o.result()
        r = dict(r, x=r["x"].cpu().numpy(), grad=r["grad"].cpu().numpy())
        _RUNS[key] = (x0, xs, fs, gs, r, o.get_trace(), n_done)
        o.close()
    return _RUNS[key]


def step_mode_equals_fit_mode(cls, N):
    """K = 4 rounds of ONE LBFGS.step (the first fresh, the others resumed) = one run_fitting with maxiters = 4 and both of its
    own tests off, bit for bit: trial points, entry losses, final point."""
    K = 4
    lb = dict(max_iter=20, max_eval=25)
    x0 = np.stack([X.family_x0(N, b) for b in range(X.NB)])
    fit = opt(cls, X.NB, N, maxiters=K, ftol=0.0, gtol=0.0, **lb)
    fit.trace(256)
    fxs, _, _, _ = drive(fit, x0, family())
    rf = fit.result()
    entry_fit = [t[t[:, 0] == 1][:, 1].astype(np.float32) for t in fit.get_trace()]
    step = opt(cls, X.NB, N, **lb)
    x, done, sxs, entry = x0, np.zeros(X.NB, np.int64), [[] for _ in range(X.NB)], []
    for k in range(K):
        rxs, _, _, _ = drive(step, x, family(), mode="step", resume=k > 0)
        rs = step.result()
        assert (rs["status"] == 1).all()
        for b in range(X.NB):
            sxs[b].append(rxs[:int(rs["evals"][b] - done[b]), b])
        done = rs["evals"].astype(np.int64)
        entry.append(rs["result"].copy())
        x = rs["x"].cpu().numpy()
    entry = np.stack(entry, 1)
    for b in range(X.NB):
        assert len(entry_fit[b]) == K and np.array_equal(bits(entry_fit[b]), bits(entry[b])), ("entry losses", b)
        assert done[b] == rf["evals"][b]
        assert np.array_equal(bits(np.concatenate(sxs[b])), bits(fxs[:done[b], b])), ("trial points", b)
    assert np.array_equal(bits(x), bits(rf["x"].cpu().numpy())), "final point"
    fit.close(); step.close()


def nan_loss_ends_one_problem_only(cls, label):
    """One problem of the batch is fed NaN as its third loss (the case and why it is this one: opt_ext_common.NAN_CONFIG): it goes
    on and ends as the machine fed the same evaluations does, and the other four never notice: bit for bit their clean run
    (family_run of the same configuration)."""
    (N, hname), bad = X.NAN_CONFIG, X.NAN_PROBLEM
    hyper = X.HYPER[hname]
    x0, xs, fs, gs, r, _, _ = family_run(cls, N, hname)

    def evaluate(xt, k):
        f, g = X.family_eval(xt)
        if k == X.NAN_AT:
            f = f.clone(); f[bad] = float("nan")
        return f, g
    o = opt(cls, X.NB, N, **hyper)
    o.trace(256)
    nxs, nfs, ngs, _ = drive(o, x0, evaluate)
    rn = o.result()
    tr = o.get_trace()
    for b in range(X.NB):
        n = int(rn["evals"][b])
        if b == bad:
            assert n > X.NAN_AT + 1 and np.isnan(nfs[X.NAN_AT, b])
            res = dict(evals=n, status=rn["status"][b], result=rn["result"][b])
            check_replay(label, "N=%d %s NaN loss trial points" % (N, hname), hyper, x0[b], nxs[:, b], nfs[:, b], ngs[:, b],
                         res, tr[b], X.bound(N, hname))
            continue
        assert n == r["evals"][b]
        assert np.array_equal(bits(nxs[:n, b]), bits(xs[:n, b])) and np.array_equal(bits(rn["result"][b]), bits(r["result"][b]))
        assert np.array_equal(bits(rn["x"].cpu().numpy()[b]), bits(r["x"][b]))
    o.close()
