"""CPU tests of the optimiser for caller-written closures (sfx_opt_*, engine.BatchOptimizer, optimizers.lbfgs_ls.LBFGS.step with
any callable): the replay design the GPU tests (test_gpu_opt_ext.py) rest on, and the refusals that need no device.

The GPU tests compare the device with oracle/lbfgs_machine.StageMachine fed the evaluations the device consumed, within
10 x the error of two arithmetic variants of the machine (tests/opt_ext_common.py).  That is a fair yardstick only where the
variants themselves stay in lock-step with the machine: where a rounding difference flips a branch, the two runs part and the
"error" measures nothing.  Every configuration the GPU tests use is therefore checked here first."""
import numpy as np
import pytest
import torch

import opt_ext_common as X


@pytest.mark.parametrize("N,hname", X.HOST_CONFIGS)
def test_variants_stay_in_lock_step(N, hname):
    """Both variants, on each of the 5 problems: the machine fed their evaluations wants every one of them and is done after the
    last; the same record types and evaluation counts per line search and per step; the same result."""
    worst = 0.0
    for b in range(X.NB):
        for name, err, lock, recs, res, n in X.yardstick(N, hname, b):
            assert lock, (N, hname, b, name, "left lock-step", n)
            assert recs, (N, hname, b, name, "records differ")
            assert res, (N, hname, b, name, "results differ")
            assert n <= 150, (N, hname, b, n)          # the GPU tests' launch counts stay small
            worst = max(worst, err)
    print("N = %d, %s: worst relative trial-point difference of the variants %.2e -> bound %.2e" % (N, hname, worst, X.bound(N, hname)))
    assert X.bound(N, hname) == max(X.FLOOR, 10 * worst)
    assert worst < 1e-3, "a variant this far from the machine is not a rounding difference"


@pytest.mark.parametrize("N,hname,distinct", X.INDEPENDENCE_CONFIGS)
def test_batch_problems_finish_at_different_evaluations(N, hname, distinct):
    """The batch-independence test on the GPU needs problems that end at different times."""
    n = [X.yardstick(N, hname, b)[0][5] for b in range(X.NB)]
    assert len(set(n)) >= distinct, n


def test_the_nan_case_has_a_reference():
    """The problem the GPU test feeds a NaN loss: the machine has a defined end there (see opt_ext_common.NAN_CONFIG), it does
    consume the NaN and goes on, and the variants stay in lock-step with it."""
    from oracle.lbfgs_machine import StageMachine
    (N, hname), b = X.NAN_CONFIG, X.NAN_PROBLEM
    assert X.NAN_CONFIG in [c[:2] for c in X.INDEPENDENCE_CONFIGS] and X.NAN_CONFIG in X.GPU_CONFIGS
    x0, hyper = X.family_x0(N, b), X.HYPER[hname]
    for name, v in X.variants(x0, **hyper):
        xs, fs, gs = X.run_on_cpu_closure(v, b, nan_at=X.NAN_AT)
        assert len(xs) > X.NAN_AT + 1 and v.result is not None and np.isfinite(v.result) and np.isfinite(v.x).all(), (name, len(xs), v.result)
        m = StageMachine(x0, dtype=np.float32, **hyper)
        err, lock = X.replay(m, xs, fs, gs)
        assert lock and X.same_records(v.records, m.records) and X.same_result(v.result, m.result), (name, lock)
        assert err <= X.bound(N, hname), (name, err, X.bound(N, hname))


@pytest.mark.parametrize("fname,N", X.GOLDEN_CASES)
def test_machine_variants_follow_the_golden_trajectories(fname, N):
    """tests/golden/lbfgs.npz, float32 runs of the reference: fed the golden's evaluations, the machine and both variants finish
    after exactly its number of evaluations, return its result and propose its points within the variants' own spread."""
    g = X.gold()
    for name, err, lock, res in X.golden_yardstick(g, fname, N):
        assert lock and res, (fname, N, name, lock, res)
        assert err < 1e-3, (fname, N, name, err)
        if name == "machine" and N == 2:
            assert err == 0.0          # order-independent dot products: bit for bit
    print("%s_%d: %s" % (fname, N, ["%s %.2e" % (e[0], e[1]) for e in X.golden_yardstick(g, fname, N)]))


def _lbfgs(params, **kw):
    from smplifyx_amd.optimizers.lbfgs_ls import LBFGS
    return LBFGS(params, line_search_fn="strong_Wolfe", **kw)


def _closure_of(params):
    def closure():
        for p in params:
            p.grad = None
        l = sum((p ** 2).sum() for p in params)
        l.backward()
        return l
    return closure


def test_step_refuses_more_than_192_elements():
    x = torch.zeros(193, requires_grad=True)
    with pytest.raises(ValueError, match="193 elements.*192"):
        _lbfgs([x]).step(_closure_of([x]))
    xs = [torch.zeros(4, 100, requires_grad=True), torch.zeros(4, 93, requires_grad=True)]
    with pytest.raises(ValueError, match="193 elements per sample"):
        _lbfgs(xs, per_sample=True).step(_closure_of(xs))


def test_step_refuses_more_than_12_tensors():
    xs = [torch.zeros(2, requires_grad=True) for _ in range(13)]
    with pytest.raises(ValueError, match="13 parameter tensors.*12"):
        _lbfgs(xs).step(_closure_of(xs))


def test_step_refuses_cpu_tensors():
    x = torch.zeros(6, requires_grad=True)
    with pytest.raises(ValueError, match="parameter 0 is on cpu.*no CPU fallback"):
        _lbfgs([x]).step(_closure_of([x]))
    assert x.grad is None and torch.equal(x.detach(), torch.zeros(6)), "a refused step touches nothing"


def test_step_refuses_other_dtypes_and_ragged_batches():
    xs = [torch.zeros(4, 3, requires_grad=True), torch.zeros(5, 3, requires_grad=True)]
    with pytest.raises(ValueError, match="same leading dimension"):
        _lbfgs(xs, per_sample=True).step(_closure_of(xs))
    with pytest.raises(TypeError, match="callable"):
        _lbfgs([xs[0]]).step(None)


def test_run_fitting_refuses_what_it_cannot_drive():
    """A plain callable needs this package's LBFGS (a torch.optim object goes with a closure of create_fitting_closure); a
    per-sample optimiser is not ONE problem."""
    from smplifyx_amd import fitting
    x = torch.zeros(6, requires_grad=True)
    mon = fitting.FittingMonitor(maxiters=3)
    with pytest.raises(TypeError, match="callable"):
        mon.run_fitting(torch.optim.SGD([x], lr=0.1), _closure_of([x]), [x], None, 0)
    with pytest.raises(NotImplementedError, match="BatchOptimizer"):
        mon.run_fitting(_lbfgs([x.reshape(1, 6)], per_sample=True), _closure_of([x]), [x], None, 0)


def test_batch_optimizer_refuses_bad_shapes_before_the_device():
    """sfx_opt_create checks its limits before it looks for a device: the refusals read the same on a machine without one."""
    from smplifyx_amd import _capi, engine
    for kw, msg in ((dict(B=1, N=193), "N = 193"), (dict(B=1, N=0), "N = 0"), (dict(B=0, N=4), "B = 0"),
                    (dict(B=1, N=13, groups=[1] * 13), "13 parameter groups"), (dict(B=1, N=6, groups=[2, 3]), "sum to 5"),
                    (dict(B=1, N=6, history_size=401), "history_size 401"), (dict(B=1, N=6, history_size=0), "history_size")):
        with pytest.raises(_capi.SfxError, match=msg):
            engine.BatchOptimizer(**kw)
    with pytest.raises(TypeError, match="unknown hyper-parameter"):
        engine.BatchOptimizer(1, 6, momentum=0.9)
    if not torch.cuda.is_available():
        with pytest.raises(_capi.SfxError, match="no HIP device"):
            engine.BatchOptimizer(1, 6)
